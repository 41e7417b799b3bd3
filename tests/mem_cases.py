"""The table of the memory-contract tests: one Case per (entry point, problem).

A Case knows how to run its qe_* entry point through an allocator (Plain: ordinary tensors; Poisoned: every buffer inside
a tests/arena.py Arena), which plan / path query names its kernel, and how its outputs compare with float64.  The problems
are the smallest ragged rows of the existing instance tables, drawn by the existing builders, so the same kernel instances
run as in the per-instance tests; only the surroundings differ.

    run(a)      -> Result(outs {name: tensor}, kernel): calls the entry point once; every operand comes from `a`.
                   `kernel` is what the plan / form / path query answers for the pointers of this very call.
    check_ref(r): the outputs of a plain call against the float64 reference, every element, the family's existing rule.
    host()      -> (instances, {workspace query: bytes}): host-only (no GPU) restatement for the coverage test.
    offsets     : {buffer name: bytes} of the second pass, for entries whose path query looks at a pointer."""
import ctypes
import functools

import numpy as np
import torch

import arena
import lin_bf16in_instances as bi
import lin_instances as li
import oracle
import test_lin_instances_gpu as tl
import test_linear_bf16_input_gpu as tb
from conftest import conv_tolerance
from quantize_amd import capi

DEV = torch.device("cuda", 0)
ALIGNED = 1 << 20        # a 256-byte aligned stand-in address for the host-only queries
EPS24 = 2.0 ** -24


# ---- allocators ------------------------------------------------------------------------------------------------------
class Plain:
    """Ordinary tensors, as every other test passes them.  offs: {buffer name: byte offset off a 256-byte boundary}."""
    fill = None

    def __init__(self, offs=None):
        self.offs = dict(offs or {})

    def _at(self, nbytes, name):
        off = self.offs.get(name, 0)
        raw = torch.empty(nbytes + off, dtype=torch.uint8, device=DEV)
        return raw[off:off + nbytes]

    def inp(self, name, t, inplace=False):
        if t is None:
            return None
        t = t.to(DEV).contiguous()
        v = self._at(t.numel() * t.element_size(), name).view(t.dtype).view(t.shape)
        v.copy_(t)
        return v

    def out(self, name, shape, dtype):
        shape = (int(shape),) if isinstance(shape, (int, np.integer)) else tuple(shape)
        n = int(np.prod(shape, dtype=np.int64)) * torch.empty((), dtype=dtype).element_size()
        return self._at(n, name).view(dtype).view(shape)

    def ws(self, name, nbytes):
        """Exactly the bytes the size query returned; None for none."""
        return self.out(name, int(nbytes), torch.uint8) if nbytes else None

    def status(self, name="status"):
        return torch.zeros(1, dtype=torch.int32, device=DEV)

    def check(self, what):
        torch.cuda.synchronize()


class Poisoned(Plain):
    def __init__(self, fill, offs=None, device=DEV):
        Plain.__init__(self, offs)
        self.fill, self.arena = fill, arena.Arena(device, fill)

    def inp(self, name, t, inplace=False):
        if t is None:
            return None
        return self.arena.place(t.to(self.arena.device), off=self.offs.get(name, 0), name=name, inplace=inplace)

    def out(self, name, shape, dtype):
        return self.arena.blank(shape, dtype, off=self.offs.get(name, 0), name=name)

    def status(self, name="status"):
        return self.arena.status(name)

    def check(self, what):
        self.arena.check(what)


class Result:
    def __init__(self, outs, kernel):
        self.outs, self.kernel = outs, kernel


class Case:
    family = fn = id = None
    expected = None          # the kernel the table records for the problem (what `kernel` must be on aligned buffers)
    offsets = None           # second pass: {buffer name: smallest offset its element type allows}
    env = None               # the row's QE_* knobs
    refused = False          # the library turns the problem down: every call raises and leaves every byte alone

    def run(self, a):
        raise NotImplementedError

    def names_expected(self, kernel):
        """`kernel`, the query's answer for aligned plain tensors, is the kernel the table records."""
        return self.expected is None or kernel == self.expected

    def check_ref(self, r):
        raise NotImplementedError

    def host(self):
        raise NotImplementedError

    def __repr__(self):
        return self.id


def _q(bits=8, n_param=1, ptr=ALIGNED):
    return capi.QeQParam(ptr, bits, 1, ALIGNED, ALIGNED, n_param)


def _within(got, ref64, bound, what):
    err = np.abs(got.astype(np.float64) - ref64)
    bad = ~(err <= bound)                                       # a NaN is bad
    print("%s: worst error %.3g, its bound %.3g" % (what, float(np.nanmax(err)), float(np.max(bound))))
    assert not bad.any(), "%s: %d of %d elements off float64, worst %.3g (bound %.3g)" % (
        what, int(bad.sum()), err.size, float(np.nanmax(err)), float(np.max(bound)))


# ---- int8 linears ----------------------------------------------------------------------------------------------------
F32, CODES, CODES_GELU, RES, RES_INPLACE, BF16 = "F32", "CODES", "CODES_GELU", "RES", "RES_INPLACE", "BF16"
LIN_FN = {F32: "qe_quantlinear", CODES: "qe_quantlinear_requant", CODES_GELU: "qe_quantlinear_requant",
          RES: "qe_quantlinear_residual", RES_INPLACE: "qe_quantlinear_residual", BF16: "qe_quantlinear_bf16"}
LIN_WS = {CODES: "qe_quantlinear_requant_workspace_bytes", CODES_GELU: "qe_quantlinear_requant_workspace_bytes",
          RES: "qe_quantlinear_residual_workspace_bytes", RES_INPLACE: "qe_quantlinear_residual_workspace_bytes",
          BF16: "qe_quantlinear_bf16_workspace_bytes"}
POST_SCALE = 0.125
MAX_B = 1024
# B = 3, K = 37, O = 5 with 3-bit x and 5-bit w: both packed streams end mid-byte (111 codes of 3 bits = 41.6 bytes, 185 of
# 5 bits = 115.6); the second with per-row x scales, so that scale[B] and zero[B] are the first floats of a guard
ODD_TAIL = [(3, 37, 5, False, "odd tails, per-tensor x"), (3, 37, 5, True, "odd tails, per-row x")]


@functools.lru_cache(maxsize=None)
def _lin_problem(key):
    """Operands, float64 value, allowance and the consumers' quantisers of one int8 row: drawn once, never changed."""
    kind, i = key
    if kind == "row":
        B, K, O, env, form, note = li.ROWS[i]
        op = tl._operands(i, B, K, O)
        x_bits = w_bits = 8
    else:
        B, K, O, per_row, note = ODD_TAIL[i]
        env, form, x_bits, w_bits = None, 0, 3, 5
        rng = np.random.RandomState(4000 + i)
        xp = oracle.tpack(rng.randint(-4, 4, size=(B, K)), x_bits, True)[0]
        wp = oracle.tpack(rng.randint(0, 32, size=(O, K)), w_bits, False)[0]
        assert (B * K * x_bits) % 8 and (O * K * w_bits) % 8
        f = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32)).to(DEV)
        nx = B if per_row else 1
        op = dict(xu=torch.from_numpy(xp).to(DEV), wu=torch.from_numpy(wp).to(DEV), xs=f(rng.uniform(1e-2, 3e-2, nx)),
                  xz=f(rng.uniform(-3, 3, nx)), ws=f(rng.uniform(2e-3, 6e-3, O)), wz=f(rng.uniform(-20, -10, O)),
                  bias=f(rng.normal(0, 0.2, O)), x_sign=True, w_sign=False)
    args = (op["xu"].cpu().numpy(), np.array([x_bits, int(op["x_sign"]), B, K]), op["xs"].cpu().numpy(), op["xz"].cpu().numpy(),
            op["wu"].cpu().numpy(), np.array([w_bits, int(op["w_sign"]), O, K]), op["ws"].cpu().numpy(), op["wz"].cpu().numpy(),
            op["bias"].cpu().numpy())
    o64 = oracle.quantlinear(*args, mode="f64", return_f64=True)[1]
    c32, cfma = oracle.quantlinear(*args, mode="fp32"), oracle.quantlinear(*args, mode="fp32_fma")
    allowed = conv_tolerance(c32, o64, c32, cfma)[1]
    p = dict(op, B=B, K=K, O=O, env=env, form=form, note=note, x_bits=x_bits, w_bits=w_bits, o64=o64, allowed=allowed)
    # the consumers' quantisers, placed from the float64 value as test_lin_instances_gpu._consumer places them from y
    y = torch.from_numpy(o64.astype(np.float32)).to(DEV)
    p["consumer"] = {act: tl._consumer(y, act) for act in (None, "gelu")}
    p["res"] = torch.randn(B, O, generator=torch.Generator(device=DEV).manual_seed(i), device=DEV)
    return p


class LinearCase(Case):
    family = "linear"

    def __init__(self, key, epi):
        self.key, self.epi = key, epi
        kind, i = key
        if kind == "row":
            B, K, O, env, form, note = li.ROWS[i]
            self.bits = (8, 8)
        else:
            B, K, O, per_row, note = ODD_TAIL[i]
            env, form = None, 0
            self.bits = (3, 5)
            self.per_row = per_row
        self.B, self.K, self.O, self.env, self.form = B, K, O, env, form
        self.fn = LIN_FN[epi]
        self.id = "%s-%dx%dx%d%s%s-%s" % (self.fn[3:], B, K, O, "-" + "-".join(env.values()) if env else "",
                                          "" if kind == "row" else "-odd%d" % i, epi)
        # what the query of this entry point names: the form for qe_quantlinear, fused (1) or two passes (0) otherwise
        self.fused = int(form != 0 and (epi != BF16 or O % 8 == 0))
        self.expected = form if epi == F32 else self.fused
        if epi in (CODES, CODES_GELU):
            self.offsets = {"codes": 1}
        elif epi == BF16:
            self.offsets = {"out": 2}

    def instances(self):
        """The template instances the case runs (names of tests/lin_instances.py)."""
        if self.form == 0 or not self.fused:
            return {(li.KERNEL[self.form], li.F32)}
        return {(li.KERNEL[self.form], RES if self.epi == RES_INPLACE else self.epi)}

    def host(self):
        B, K, O = self.B, self.K, self.O
        L = capi.lib()
        xq, wq = _q(self.bits[0]), _q(self.bits[1])
        with capi.knobs(**(self.env or {})):
            assert capi.linear_form(xq, wq, B, K, O) == self.form, self.id
            rq = capi.QeRequant(ALIGNED, ALIGNED, 1, -128.0, 127.0, 8, 1)
            ws = {}
            if self.epi in (CODES, CODES_GELU):
                assert int(L.qe_quantlinear_requant_path(xq, wq, B, K, O, rq, ALIGNED)) == self.fused, self.id
                ws[LIN_WS[self.epi]] = int(L.qe_quantlinear_requant_workspace_bytes(xq, wq, B, K, O, rq, ALIGNED))
            elif self.epi in (RES, RES_INPLACE):
                assert capi.linear_residual_path(xq, wq, B, K, O) == self.fused, self.id
                ws[LIN_WS[self.epi]] = int(L.qe_quantlinear_residual_workspace_bytes(xq, wq, B, K, O))
            elif self.epi == BF16:
                assert int(L.qe_quantlinear_bf16_path(xq, wq, B, K, O, ALIGNED)) == self.fused, self.id
                ws[LIN_WS[self.epi]] = int(L.qe_quantlinear_bf16_workspace_bytes(xq, wq, B, K, O, ALIGNED))
        return self.instances(), ws

    def run(self, a):
        p = _lin_problem(self.key)
        B, K, O, epi = self.B, self.K, self.O, self.epi
        L = capi.lib()
        xq = capi.qparam(a.inp("x", p["xu"]), p["x_bits"], p["x_sign"], a.inp("x scale", p["xs"]), a.inp("x zero", p["xz"]))
        wq = capi.qparam(a.inp("w", p["wu"]), p["w_bits"], p["w_sign"], a.inp("w scale", p["ws"]), a.inp("w zero", p["wz"]))
        bias = a.inp("bias", p["bias"])
        with capi.knobs(**(self.env or {})):
            if epi == F32:
                out = a.out("out", (B, O), torch.float32)
                kernel = capi.linear_form(xq, wq, B, K, O, dst_aligned=out.data_ptr() % 16 == 0)
                capi.quantlinear(xq, wq, bias, B, K, O, out=out)
                return Result({"out": out}, kernel)
            if epi in (CODES, CODES_GELU):
                act = "gelu" if epi == CODES_GELU else None
                rq0, _, _, qmin, qmax = p["consumer"][act]
                rq = capi.requant(a.inp("rq scale", rq0._keep[0]), a.inp("rq zero", rq0._keep[1]), qmin, qmax, 8, rq0.sign)
                codes, status = a.out("codes", B * O, torch.uint8), a.status()
                kernel = capi.linear_requant_path(xq, wq, B, K, O, rq, codes)
                need = int(L.qe_quantlinear_requant_workspace_bytes(xq, wq, B, K, O, rq, codes.data_ptr()))
                capi.quantlinear_requant(xq, wq, bias, B, K, O, rq, act=act, codes=codes, status=status,
                                         workspace=a.ws("workspace", need))
                return Result({"codes": codes, "status": status}, kernel)
            if epi in (RES, RES_INPLACE):
                res = a.inp("residual", p["res"], inplace=epi == RES_INPLACE)
                out = res if epi == RES_INPLACE else a.out("out", (B, O), torch.float32)
                kernel = capi.linear_residual_path(xq, wq, B, K, O)
                need = int(L.qe_quantlinear_residual_workspace_bytes(xq, wq, B, K, O))
                capi.quantlinear_residual(xq, wq, bias, B, K, O, res, out=out, workspace=a.ws("workspace", need))
                return Result({"out": out}, kernel)
            out = a.out("out", (B, O), torch.bfloat16)
            kernel = capi.quantlinear_bf16_path(xq, wq, B, K, O, out)
            need = int(L.qe_quantlinear_bf16_workspace_bytes(xq, wq, B, K, O, out.data_ptr()))
            capi.quantlinear_bf16(xq, wq, bias, B, K, O, post_scale=POST_SCALE, out=out, workspace=a.ws("workspace", need))
            return Result({"out": out}, kernel)

    def check_ref(self, r):
        """Every element against float64.  `allowed` is conv_tolerance's allowance of the row (the oracle's own fp32 chains
        against its float64 value); the fused epilogues are held to the float64 value of their own result, not to a
        two-pass form of the same y:
          RES   out = fl(y + res): |out - (y64 + res)| <= allowed + 2^-24 (|y64 + res| + allowed)
          BF16  out = bf16(fl(y s)): one fp32 and one bf16 rounding, relative 2^-24 and 2^-8 (8 significant bits)
          CODES test_lin_instances_gpu._check_codes_vs_f64 (a flip of one only inside the tie band), status 0."""
        p = _lin_problem(self.key)
        o64, allowed, epi = p["o64"], p["allowed"], self.epi
        if epi == F32:
            _within(r.outs["out"].cpu().numpy(), o64, allowed, self.id)
        elif epi in (RES, RES_INPLACE):
            v = o64 + p["res"].cpu().numpy().astype(np.float64)
            _within(r.outs["out"].cpu().numpy(), v, allowed + EPS24 * (np.abs(v) + allowed), self.id)
        elif epi == BF16:
            v = o64 * POST_SCALE
            a = POST_SCALE * allowed
            _within(r.outs["out"].float().cpu().numpy(), v, a + (2.0 ** -8 + EPS24) * (np.abs(v) + a), self.id)
        else:
            act = "gelu" if epi == CODES_GELU else None
            rq, sc, zr, qmin, qmax = p["consumer"][act]
            assert int(r.outs["status"].item()) == 0, self.id
            cq = tl._stored_to_q(r.outs["codes"].view(self.B, self.O), rq.sign).cpu().numpy()
            v64 = tl._gelu64(o64) if act == "gelu" else o64
            tl._check_codes_vs_f64(cq, v64, allowed, act, sc, zr, qmin, qmax, self.id)


# ---- float-input and bf16-input linears ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _flin_problem(i):
    """Row i of lin_instances.F_ROWS, drawn as test_lin_instances_gpu.test_float_input_row_every_epilogue draws it."""
    B, K, O, env, form, note = li.F_ROWS[i]
    g = torch.Generator(device=DEV).manual_seed(2000 + i)
    x = torch.randn(B, K, generator=g, device=DEV)
    wu = torch.randint(0, 256, (O, K), dtype=torch.uint8, generator=g, device=DEV)
    ws = torch.rand(O, generator=g, device=DEV) * 4e-3 + 2e-3
    wz = torch.rand(O, generator=g, device=DEV) * 4 - 2
    bias = torch.randn(O, generator=g, device=DEV) * 0.2
    res = torch.randn(B, O, generator=g, device=DEV)
    p = dict(x=x, wu=wu, ws=ws, wz=wz, bias=bias, res=res, sign=True, w_bits=8)
    p["o64"], c32, cfma = tb._oracle(p, x.cpu().numpy(), K, O)
    p["allowed"] = conv_tolerance(c32, p["o64"], c32, cfma)[1]
    return p


@functools.lru_cache(maxsize=None)
def _blin_problem(i):
    B, K, O, w_bits, off, path, note = bi.ROWS[i]
    p = tb._problem(i)
    p["o64"], c32, cfma = tb._oracle(p, p["x"].float().cpu().numpy(), K, O)
    p["allowed"] = conv_tolerance(c32, p["o64"], c32, cfma)[1]
    p["res"] = torch.randn(B, O, generator=torch.Generator(device=DEV).manual_seed(i), device=DEV)
    return p


class FloatLinearCase(Case):
    """qe_quantlinear_float_input[_residual] on a row of F_ROWS, or qe_quantlinear_bf16_input on a row of
    lin_bf16in_instances.ROWS (bf16=True), with and without a residual."""
    family = "linear"

    def __init__(self, i, residual, bf16=False):
        self.i, self.residual, self.bf16 = i, residual, bf16
        if bf16:
            B, K, O, self.w_bits, self.x_off, path, note = bi.ROWS[i]
            self.env = None
            self.fn = "qe_quantlinear_bf16_input"
            self.expected = path
            self.offsets = {"x": 2} if self.x_off == 0 else None
        else:
            B, K, O, self.env, form, note = li.F_ROWS[i]
            self.w_bits, self.x_off = 8, 0
            self.fn = "qe_quantlinear_float_input" + ("_residual" if residual else "")
            self.expected = form
        self.B, self.K, self.O = B, K, O
        self.id = "%s-%dx%dx%d%s%s%s" % (self.fn[3:], B, K, O, "-" + "-".join(self.env.values()) if self.env else "",
                                         "-w%d" % self.w_bits if self.w_bits != 8 else "",
                                         ("-off%d" % self.x_off if self.x_off else "") + ("-res" if residual and bf16 else ""))

    def instances(self):
        epi = RES if self.residual else F32
        if self.bf16:
            return {(li.B_KERNEL, epi)} if self.expected == 1 else set()
        return {(li.F_KERNEL[self.expected], epi if self.expected == 1 else F32)}

    def host(self):
        B, K, O = self.B, self.K, self.O
        L = capi.lib()
        wq = _q(self.w_bits)
        ws = {}
        with capi.knobs(**(self.env or {})):
            if self.bf16:
                x = ALIGNED + self.x_off
                assert int(L.qe_quantlinear_bf16_input_path(x, wq, B, K, O)) == self.expected, self.id
                ws["qe_quantlinear_bf16_input_workspace_bytes"] = int(L.qe_quantlinear_bf16_input_workspace_bytes(x, wq, B, K, O))
            else:
                assert int(L.qe_quantlinear_float_input_path(ALIGNED, wq, B, K, O)) == self.expected, self.id
                if self.residual:
                    assert int(L.qe_quantlinear_float_input_residual_path(ALIGNED, wq, B, K, O)) == self.expected, self.id
                    ws["qe_quantlinear_float_input_residual_workspace_bytes"] = int(
                        L.qe_quantlinear_float_input_residual_workspace_bytes(ALIGNED, wq, B, K, O))
        return self.instances(), ws

    def run(self, a):
        p = _blin_problem(self.i) if self.bf16 else _flin_problem(self.i)
        B, K, O = self.B, self.K, self.O
        L = capi.lib()
        if self.bf16 and self.x_off:
            a.offs.setdefault("x", self.x_off)
        x = a.inp("x", p["x"])
        wq = capi.qparam(a.inp("w", p["wu"]), self.w_bits, p["sign"], a.inp("w scale", p["ws"]), a.inp("w zero", p["wz"]))
        bias = a.inp("bias", p["bias"])
        res = a.inp("residual", p["res"]) if self.residual else None
        out = a.out("out", (B, O), torch.float32)
        with capi.knobs(**(self.env or {})):
            if self.bf16:
                kernel = capi.quantlinear_bf16_input_path(x, wq, B, K, O)
                need = int(L.qe_quantlinear_bf16_input_workspace_bytes(x.data_ptr(), wq, B, K, O))
                capi.quantlinear_bf16_input(x, wq, bias, O, residual=res, out=out, workspace=a.ws("workspace", need))
            elif self.residual:
                kernel = capi.linear_float_input_residual_path(x, wq, B, K, O)
                need = int(L.qe_quantlinear_float_input_residual_workspace_bytes(x.data_ptr(), wq, B, K, O))
                capi.quantlinear_float_input_residual(x, wq, bias, O, res, out=out, workspace=a.ws("workspace", need))
            else:
                kernel = capi.linear_float_input_path(x, wq, B, K, O)
                capi.quantlinear_float_input(x, wq, bias, O, out=out)
        return Result({"out": out}, kernel)

    def check_ref(self, r):
        """conv_tolerance on the widened rows; with a residual one more fp32 rounding of the sum (as LinearCase RES)."""
        p = _blin_problem(self.i) if self.bf16 else _flin_problem(self.i)
        v, allowed = p["o64"], p["allowed"]
        bound = allowed
        if self.residual:
            v = v + p["res"].cpu().numpy().astype(np.float64)
            bound = allowed + EPS24 * (np.abs(v) + allowed)
        _within(r.outs["out"].cpu().numpy(), v, bound, self.id)


def linear_cases():
    out = []
    for i, row in enumerate(li.ROWS):
        if row[0] <= MAX_B:
            out += [LinearCase(("row", i), e) for e in (F32, CODES, CODES_GELU, RES, RES_INPLACE, BF16)]
    for i in range(len(ODD_TAIL)):
        out += [LinearCase(("odd", i), e) for e in (F32, CODES, RES, BF16)]
    for i, row in enumerate(li.F_ROWS):
        if row[0] <= MAX_B:
            out += [FloatLinearCase(i, False), FloatLinearCase(i, True)]
    for i, row in enumerate(bi.ROWS):
        if row[0] <= MAX_B:
            out += [FloatLinearCase(i, False, bf16=True), FloatLinearCase(i, True, bf16=True)]
    return out


# ---- LayerNorm, patchify, pools --------------------------------------------------------------------------------------
LN_ROWS, LN_EPS = 5, 1e-6
# (scale, zero, bits, signed) of the consumers: "3" is three 8-bit per-tensor ones (the kernel writes all codes itself),
# "3low" ends in a 4-bit one (two passes: the LayerNorm goes through the workspace when there is no ln_out)
LN_RQS = {0: [], 1: [(0.02, 0.0, 8, True)], "3": [(0.02, 0.0, 8, True), (0.03, -120.0, 8, False), (0.025, 3.0, 8, True)],
          "3low": [(0.03, 0.0, 8, True), (0.05, -100.0, 8, False), (0.4, 1.0, 4, True)]}


@functools.lru_cache(maxsize=None)
def _ln_problem(E):
    import test_vit_ops_gpu as tv
    x, gamma, beta = tv._ln_input(LN_ROWS, E, seed=LN_ROWS * 4096 + E)
    if E % 4:
        return dict(x=x, gamma=gamma, beta=beta)
    ref = tv._ln64(x, gamma, beta, LN_EPS)
    return dict(x=x, gamma=gamma, beta=beta, ref=ref, bound=tv._ln_bound(ref, x, gamma, beta, LN_EPS))


class LayerNormCase(Case):
    family = "ew"
    fn = "qe_layernorm_quantize_pack"

    def __init__(self, E, n_out, with_ln):
        self.E, self.n_out, self.with_ln = E, n_out, with_ln
        self.rqs = LN_RQS[n_out]
        self.refused = E % 4 != 0                    # E = 66: no kernel takes it; the call must leave every byte alone
        self.id = "layernorm-%dx%d-%s-%s" % (LN_ROWS, E, "rq%s" % n_out, "ln" if with_ln else "codes")
        if not self.refused and n_out:
            self.expected = 0 if n_out == "3low" else 1
            self.offsets = {"codes0": 1}

    def host(self):
        L = capi.lib()
        arr = capi._rq_array([capi.QeRequant(ALIGNED, ALIGNED, 1, 0.0, 15.0, b, int(s)) for _, _, b, s in self.rqs])
        cp = (ctypes.c_void_p * max(1, len(self.rqs)))(*[ALIGNED] * len(self.rqs))
        if self.expected is not None:
            assert int(L.qe_layernorm_quantize_pack_path(LN_ROWS, self.E, len(self.rqs), arr, cp)) == self.expected, self.id
        need = int(L.qe_layernorm_quantize_pack_workspace_bytes(LN_ROWS, self.E, len(self.rqs), arr, cp,
                                                                ALIGNED if self.with_ln else None))
        return {("layernorm", self.E, self.expected)}, {"qe_layernorm_quantize_pack_workspace_bytes": need}

    def run(self, a):
        p = _ln_problem(self.E)
        E, L = self.E, capi.lib()
        x, gamma, beta = a.inp("x", p["x"]), a.inp("gamma", p["gamma"]), a.inp("beta", p["beta"])
        f = lambda v: torch.tensor([v], dtype=torch.float32, device=DEV)
        rqs, codes = [], []
        for k, (sc, zr, bits, sign) in enumerate(self.rqs):
            qmin, qmax = (-(1 << (bits - 1)), (1 << (bits - 1)) - 1) if sign else (0, (1 << bits) - 1)
            rqs.append(capi.requant(a.inp("rq%d scale" % k, f(sc)), a.inp("rq%d zero" % k, f(zr)), qmin, qmax, bits, sign))
            codes.append(a.out("codes%d" % k, capi.packed_nbytes(LN_ROWS * E, bits), torch.uint8))
        ln_out = a.out("ln_out", (LN_ROWS, E), torch.float32) if self.with_ln else None
        status = a.status()
        arr = capi._rq_array(rqs)
        cp = (ctypes.c_void_p * max(1, len(codes)))(*[c.data_ptr() for c in codes])
        kernel = capi.layernorm_path(LN_ROWS, E, rqs, codes)
        need = int(L.qe_layernorm_quantize_pack_workspace_bytes(LN_ROWS, E, len(rqs), arr, cp, capi._ptr(ln_out)))
        capi.layernorm_quantize_pack(x, gamma, beta, LN_EPS, rqs, ln_out=ln_out, codes=codes, status=status,
                                     workspace=a.ws("workspace", need))
        outs = {"codes%d" % k: c for k, c in enumerate(codes)}
        outs["status"] = status
        if ln_out is not None:
            outs["ln_out"] = ln_out
        return Result(outs, kernel)

    def check_ref(self, r):
        """test_vit_ops_gpu's rules: the fp32 LayerNorm within _ln_bound of float64 per row; the codes those of the float64
        value but for flips of one inside the tie band (_check_ln_codes_f64, here for any width)."""
        import ew_ref
        p = _ln_problem(self.E)
        ref, bound = p["ref"], p["bound"]
        assert int(r.outs["status"].item()) == 0, self.id
        if self.with_ln:
            e_k = (r.outs["ln_out"].double() - ref).abs().amax(-1)
            assert bool((e_k <= bound).all()), "%s: row errors %s > %s" % (self.id, e_k.tolist(), bound.tolist())
            assert torch.equal(r.outs["ln_out"][1], p["beta"])           # the constant row
        for k, (sc, zr, bits, sign) in enumerate(self.rqs):
            sc, zr = float(np.float32(sc)), float(np.float32(zr))
            qmin, qmax = (-(1 << (bits - 1)), (1 << (bits - 1)) - 1) if sign else (0, (1 << bits) - 1)
            stored = ew_ref.unpack_codes(r.outs["codes%d" % k].cpu().numpy(), ref.numel(), bits).astype(np.int64)
            q = torch.from_numpy(stored - ((1 << (bits - 1)) if sign else 0)).view(ref.shape).to(ref.device)
            t = ref / sc - zr
            q64 = torch.clamp(torch.round(t), qmin, qmax)
            d = (q.double() - q64).abs()
            band = bound[:, None] / sc + 4 * tl.EPS32 * (t.abs() + abs(zr))
            near_tie = ((t - torch.floor(t)) - 0.5).abs() <= band
            bad = (d > 1) | ((d == 1) & ~near_tie)
            assert not bool(bad.any()), "%s: %d of codes%d off the float64 codes outside the tie band" % (self.id, int(bad.sum()), k)


class PatchifyCase(Case):
    """qe_quantize_patchify, N = 2, C = 3, 32 x 32, patch 16: ew_ref.quantise's fp32 sequence on tie-dense pixels, bit for bit."""
    family = "ew"
    fn = "qe_quantize_patchify"
    N, C, H, W, P = 2, 3, 32, 32, 16

    def __init__(self, bits, sign, per_ch):
        self.bits, self.sign, self.per_ch = bits, sign, per_ch
        self.id = "patchify-b%d%s-%s" % (bits, "s" if sign else "u", "channel" if per_ch else "tensor")

    def host(self):
        return set(), {}

    @functools.lru_cache(maxsize=None)
    def problem(self):
        import ew_instances as ei
        import ew_ref
        N, C, H, W, P = self.N, self.C, self.H, self.W, self.P
        qmin, qmax = ew_ref.qrange(self.bits, self.sign)
        scale, zero = ei.channel_params(C) if self.per_ch else ei.tensor_params(self.bits)
        n = N * C * H * W
        x = ew_ref.tie_dense(np.random.RandomState(self.bits), n, scale, zero, qmin, qmax, H * W)
        q = ew_ref.patch_matrix(ew_ref.quantise(x, scale, zero, qmin, qmax, H * W).reshape(N, C, H, W), P).reshape(-1)
        return x.reshape(N, C, H, W), scale, zero, ew_ref.pack(ew_ref.stored(q, self.bits, self.sign), self.bits)

    def run(self, a):
        import ew_ref
        x, scale, zero, _ = self.problem()
        qmin, qmax = ew_ref.qrange(self.bits, self.sign)
        out, status = a.out("codes", capi.packed_nbytes(x.size, self.bits), torch.uint8), a.status()
        capi.quantize_patchify(a.inp("x", torch.from_numpy(x)), self.P, a.inp("scale", torch.from_numpy(scale)),
                               a.inp("zero", torch.from_numpy(zero)), qmin, qmax, self.bits, self.sign, out=out, status=status)
        return Result({"codes": out, "status": status}, None)

    def check_ref(self, r):
        assert int(r.outs["status"].item()) == 0, self.id
        assert np.array_equal(r.outs["codes"].cpu().numpy(), self.problem()[3]), self.id


class AvgPoolCase(Case):
    """qe_global_avgpool on 3 planes of 49: test_ew_instances_pool_gpu's bound, (P + 1) 2^-24 mean|x| per plane."""
    family = "ew"
    fn = "qe_global_avgpool"
    id = "global_avgpool-3x49"

    def host(self):
        return set(), {}

    def run(self, a):
        x = (np.random.RandomState(49).normal(0, 1, size=(1, 3, 7, 7)) + 1e3).astype(np.float32)
        out = a.out("out", (1, 3), torch.float32)
        capi.global_avgpool(a.inp("x", torch.from_numpy(x)), out=out)
        self.x = x
        return Result({"out": out}, None)

    def check_ref(self, r):
        import ew_ref
        x = self.x
        bound = 50 * EPS24 * np.abs(x.astype(np.float64)).mean(axis=(2, 3))
        _within(r.outs["out"].cpu().numpy(), ew_ref.avgpool64(x), bound, self.id)


class MaxPoolCase(Case):
    """qe_maxpool2d_codes, N = 1, C = 3, 9 x 9, kernel 3, stride 2, padding 1: the first and the last window of every row and
    column hang over the plane's edge, where the next plane's codes (or a guard's 255) lie."""
    family = "ew"
    fn = "qe_maxpool2d_codes"
    id = "maxpool2d_codes-1x3x9x9-k3s2p1"

    def host(self):
        return set(), {}

    def run(self, a):
        codes = np.random.RandomState(81).randint(0, 200, size=(1, 3, 9, 9)).astype(np.uint8)
        out = a.out("out", 3 * 5 * 5, torch.uint8)
        capi.maxpool2d_codes(a.inp("x", torch.from_numpy(codes)), 8, 1, 3, 9, 9, 3, 2, 1, out=out)
        self.codes = codes
        return Result({"out": out}, None)

    def check_ref(self, r):
        import ew_ref
        assert np.array_equal(r.outs["out"].cpu().numpy(), ew_ref.maxpool_codes(self.codes, False, 3, 2, 1).reshape(-1)), self.id


def ew_cases():
    out = []
    for E in (66, 768):
        out += [LayerNormCase(E, n, ln) for n in (0, 1, "3", "3low") for ln in (True, False) if n or ln]
    out += [PatchifyCase(8, True, False), PatchifyCase(3, False, True)]
    return out + [AvgPoolCase(), MaxPoolCase()]


# ---- attention -------------------------------------------------------------------------------------------------------
ATTN_FN = {"fp32": "qe_attention", "masked": "qe_attention_masked", "bf16": "qe_attention_bf16",
           "stored": "qe_attention_bf16_stored", "ctx": "qe_attention_bf16_ctx"}
ATTN_KERNEL = {"bf16": "attn_bf16_kernel", "stored": "attn_bf16_stored_kernel", "ctx": "attn_bf16_ctx_kernel"}
ATTN_MFMA_D, ATTN_VALU_D = (16, 64, 128), (20, 256)


@functools.lru_cache(maxsize=None)
def _attn_problem(d, S, masked, rounded):
    """q, k, v (host, (N, T, H, d)), the operands and the float64 reference of one geometry: attn_instances' own."""
    import attention_ref as ar
    import attn_bf16_ref as br
    import attn_instances as ai
    import test_attention_gpu as base
    q, k, v = base._inputs(ai.N, ai.L, S, ai.H, d, "moderate", seed=d + S)
    ops = {}
    if masked:
        kernel = ai.MFMA if d in ai.MFMA_D else ai.VALU
        (row,) = [r for r in ai.ROWS if r[:6] == (kernel, d, S, True, True, True)]
        ops = ai.operands(row)
        assert ar.visible(ar.merged(ai.N, ai.H, ai.L, S, **ops)).all()
    p = dict(ops=ops)
    if rounded is None:                              # the fp32 core
        p.update(q=q, k=k, v=v, ref=ar.ref64(q, k, v, **ops))
    else:
        if rounded:                                  # bf16 rows as stored: the inputs are bf16 values already
            q, k, v = (br.bf16(a) for a in (q, k, v))
        qh, kh, vh = br.rounded(q, k, v)
        p.update(q=q, k=k, v=v, ref=br.ref64(qh, kh, vh, **ops), bound=br.bound(vh))
    return p


class AttentionCase(Case):
    family = "attention"

    def __init__(self, entry, d, S, masked, layout):
        import attn_instances as ai
        self.entry, self.d, self.S, self.masked, self.layout = entry, d, S, masked, layout
        self.fn = ATTN_FN[entry]
        self.expected = 2 if entry in ATTN_KERNEL else (1 if d in ai.MFMA_D else 0)
        self.id = "%s-d%d-S%d-%s-%s" % (self.fn[3:], d, S, "mask+bias+causal" if masked else "plain", layout)

    def _path(self):
        import attn_instances as ai
        m = self.masked
        q = {"fp32": lambda: capi.attention_path(ai.L, self.S, ai.H, self.d),
             "masked": lambda: capi.attention_masked_path(ai.L, self.S, ai.H, self.d, m, m, m),
             "bf16": lambda: capi.attention_bf16_path(ai.L, self.S, ai.H, self.d, m, m, m),
             "stored": lambda: capi.attention_bf16_stored_path(ai.L, self.S, ai.H, self.d, m, m, m),
             "ctx": lambda: capi.attention_bf16_ctx_path(ai.L, self.S, ai.H, self.d, m, m, m)}
        return q[self.entry]()

    def host(self):
        import attn_instances as ai
        assert self._path() == self.expected, self.id
        if self.entry in ATTN_KERNEL:
            return {(ATTN_KERNEL[self.entry], self.d)}, {}
        m = self.masked
        kind = [r for r in ai.ROWS if r[:6] == (ai.MFMA if self.expected else ai.VALU, self.d, self.S, m, m, m)][0][6]
        return {ai.instance(ai.MFMA if self.expected else ai.VALU, self.d, self.S, m, m, m, *ai.mask_strides(kind, self.S))}, {}

    def run(self, a):
        import attn_instances as ai
        import test_attention_gpu as base
        stored = self.entry in ("stored", "ctx")
        p = _attn_problem(self.d, self.S, self.masked, None if self.entry in ("fp32", "masked") else stored)
        rows = lambda x: base._rows(x, self.layout).to(torch.bfloat16) if stored else base._rows(x, self.layout)
        q, k, v = a.inp("q", rows(p["q"])), a.inp("k", rows(p["k"])), a.inp("v", rows(p["v"]))
        t = lambda name: a.inp(name, torch.from_numpy(np.ascontiguousarray(p["ops"][name]))) if name in p["ops"] else None
        out_dtype = torch.bfloat16 if self.entry == "ctx" else torch.float32
        out = a.out("out", (ai.N * ai.L, ai.H * self.d), out_dtype)
        capi.attention(q, k, v, ai.N, ai.L, ai.H, S=self.S, layout=self.layout, out=out, mask=t("mask"), key_bias=t("key_bias"),
                       causal=bool(p["ops"].get("causal", False)), precision="fp32" if self.entry in ("fp32", "masked") else "bf16",
                       out_dtype=out_dtype if self.entry == "ctx" else None)
        return Result({"out": out}, self._path())

    def check_ref(self, r):
        """The attention cores' existing bounds: fp32 e_q <= max(4 e_t, 1e-6 max|V|) and <= 1e-5 max|V| with e_t torch's fp32
        SDPA error on the same merged mask; bf16 (2^-8 + 1e-5) max|v^| against float64 on the rounded inputs; the bf16 context
        one more rounding to 8 significant bits of that."""
        import attention_ref as ar
        import attn_instances as ai
        import test_attention_gpu as base
        import test_attention_mask_gpu as mg
        stored = self.entry in ("stored", "ctx")
        p = _attn_problem(self.d, self.S, self.masked, None if self.entry in ("fp32", "masked") else stored)
        got = base._unrows(r.outs["out"].float(), ai.N, ai.L, ai.H, self.d, self.layout)
        ref = p["ref"]
        assert np.isfinite(got).all() and np.isfinite(ref).all(), self.id
        if self.entry in ("fp32", "masked"):
            merged = ar.merged(ai.N, ai.H, ai.L, self.S, **p["ops"]) if self.masked else None
            e_t = float(np.abs(mg._torch_sdpa(p["q"], p["k"], p["v"], merged) - ref).max())
            vmax = float(np.abs(p["v"]).max())
            e_q = float(np.abs(got - ref).max())
            print("%s: e_q %.3g e_t %.3g (max|V| %.3g)" % (self.id, e_q, e_t, vmax))
            assert e_q <= max(4 * e_t, 1e-6 * vmax) and e_q <= 1e-5 * vmax, (self.id, e_q, e_t)
        elif self.entry == "ctx":
            _within(got, ref, p["bound"] + 2.0 ** -8 * (np.abs(ref) + p["bound"]), self.id)
        else:
            _within(got, ref, p["bound"], self.id)


def attention_cases():
    import attn_instances as ai
    out = []
    for layout in ("token", "seq"):
        for d in ATTN_MFMA_D + ATTN_VALU_D:
            out.append(AttentionCase("fp32", d, ai.S_SCALAR, False, layout))
            out += [AttentionCase("masked", d, S, True, layout) for S in ((ai.S_SCALAR, ai.S_VEC4) if d in ATTN_MFMA_D else (ai.S_SCALAR,))]
        for entry in ("bf16", "stored", "ctx"):
            for d in ATTN_MFMA_D:
                out.append(AttentionCase(entry, d, ai.S_SCALAR, False, layout))
                out += [AttentionCase(entry, d, S, True, layout) for S in (ai.S_SCALAR, ai.S_VEC4)]
    return out


# ---- int8 convolutions -----------------------------------------------------------------------------------------------
PLAN_FIELDS = ("route", "fused", "family", "cfg", "niw", "kkt", "ns", "split", "wraw", "rq", "patch", "pre", "sub2_log_up",
               "expand", "sub_x4", "fd_w8", "pwr_tw", "pwr_ks", "pwr_groups", "pwr7_gi", "pwr_s2")


def _plan_key(info):
    """What a conv plan says about the kernels a call launches, without the sizes."""
    return tuple(int(getattr(info, f)) for f in PLAN_FIELDS)


def _conv_macs(shape):
    N, IC, H, W, OC, K, stride, pad = shape
    return N * OC * ((H + 2 * pad - K) // stride + 1) * ((W + 2 * pad - K) // stride + 1) * IC * K * K


def _qparam_host(bits):
    return capi.QeQParam(ALIGNED, bits, 1, ALIGNED, ALIGNED, 1)


def _rq_host():
    return capi.QeRequant(ALIGNED, ALIGNED, 1, -128.0, 127.0, 8, 1)


# RESIDUAL: fp32 out and the consumer's codes; RESIDUAL_F32: fp32 out only (no quantiser: the RES instance without RQ)
DIRECT, PREPARED, REQUANT, RESIDUAL, RESIDUAL_F32 = "direct", "prepared", "requant", "residual", "residual_f32"
CONV_FN = {DIRECT: "qe_quantconv2d", PREPARED: "qe_quantconv2d_prepared", REQUANT: "qe_quantconv2d_requant_prepared",
           RESIDUAL: "qe_quantconv2d_residual_prepared", RESIDUAL_F32: "qe_quantconv2d_residual_prepared"}


class ConvCase(Case):
    """One int8 conv problem through one entry point.  table "mfma": row i of conv_instances.ROWS, drawn as
    test_conv_instances_gpu._case(i, 1) draws it; table "pwr": row i of pwr_instances.ROWS, drawn as
    test_requant_gpu.test_requant_every_pwr_instance draws its rows."""
    family = "conv"

    def __init__(self, table, i, entry, env=None):
        import conv_instances as ci
        import pwr_instances as pi
        self.table, self.i, self.entry = table, i, entry
        if table == "mfma":
            self.shape, self.xb, self.wb, renv, self.inst, note = ci.ROWS[i]
        else:
            self.shape, self.inst, note, renv = pi.ROWS[i]
            self.xb = self.wb = 8
        self.env = dict(renv or {}) if env is None else dict(env)
        self.fn = CONV_FN[entry]
        extra = {k: v for k, v in self.env.items() if (renv or {}).get(k) != v}
        self.id = "%s-%s%d-%s%s%s" % (self.fn[3:], table, i, "x".join(str(v) for v in self.shape),
                                      "".join("-%s=%s" % kv for kv in sorted(extra.items())), "-f32" if entry == RESIDUAL_F32 else "")
        if entry == REQUANT:
            self.offsets = {"codes": 1}

    def _sh(self):
        N, IC, H, W, OC, K, stride, pad = self.shape
        return capi.conv_shape(N, IC, H, W, OC, K, K, stride, pad)

    # -- host only --
    def host_plan(self, codes=ALIGNED):
        with capi.knobs(**self.env):
            return capi.conv_plan_info(self._sh(), _qparam_host(self.xb), _qparam_host(self.wb),
                                       _rq_host() if self.entry in (REQUANT, RESIDUAL) else None, ALIGNED,
                                       codes if self.entry in (REQUANT, RESIDUAL) else 0)

    def instances(self):
        import conv_instances as ci
        import pwr_instances as pi
        info = self.host_plan()
        if self.table == "pwr":
            assert capi.CONV_ROUTES[info.route] in ("pwr", "pwr7") and (info.fused or self.entry in (PREPARED, RESIDUAL_F32)), self.id
            assert pi.instance(self.shape) == self.inst
            return {pi.full(self.inst, self.entry in (REQUANT, RESIDUAL), self.entry in (RESIDUAL, RESIDUAL_F32))}
        return ci.launched(info)

    def host(self):
        L = capi.lib()
        sh, xq, wq, rq = self._sh(), _qparam_host(self.xb), _qparam_host(self.wb), _rq_host()
        ws = {}
        with capi.knobs(**self.env):
            if self.entry == DIRECT:
                ws["qe_quantconv2d_workspace_bytes"] = capi.workspace_bytes(sh, self.xb, self.wb)
            else:
                ws["qe_conv_prepared_bytes"] = int(L.qe_conv_prepared_bytes(ctypes.byref(sh), self.xb, self.wb))
            if self.entry == PREPARED:
                ws["qe_quantconv2d_prepared_workspace_bytes"] = int(L.qe_quantconv2d_prepared_workspace_bytes(ctypes.byref(sh), self.xb, self.wb))
            elif self.entry == REQUANT:
                ws["qe_quantconv2d_requant_workspace_bytes"] = int(L.qe_quantconv2d_requant_workspace_bytes(
                    ctypes.byref(sh), ctypes.byref(xq), ctypes.byref(wq), ctypes.byref(rq)))
            elif self.entry in (RESIDUAL, RESIDUAL_F32):
                ws["qe_quantconv2d_residual_workspace_bytes"] = capi.residual_workspace_bytes(sh, xq, wq, rq if self.entry == RESIDUAL else None)
        return self.instances(), ws

    def names_expected(self, kernel):
        """The plan of the aligned call launches the instance the table records (the plain fp32 instance of a
        conv_instances row; any epilogue of a resident-tile row: its route and tile)."""
        import conv_instances as ci
        info = self.host_plan()
        if kernel[:len(PLAN_FIELDS)] != _plan_key(info):
            return False
        if self.table == "pwr":
            return capi.CONV_ROUTES[info.route] in ("pwr", "pwr7") and bool(info.fused or self.entry in (PREPARED, RESIDUAL_F32))
        return self.entry in (REQUANT, RESIDUAL, RESIDUAL_F32) or self.inst in ci.launched(info)

    def problem(self):
        return _conv_problem(self.table, self.i)

    def run(self, a):
        p = self.problem()
        case, L, sh = p["case"], capi.lib(), self._sh()
        T = lambda v: None if v is None else torch.from_numpy(np.ascontiguousarray(v))
        xp, xd, sx, zx = case["x"]
        wp, wd, sw, zw = case["w"]
        xq = capi.qparam(a.inp("x", T(xp)), int(xd[0]), int(xd[1]), a.inp("x scale", T(sx)), a.inp("x zero", T(zx)))
        wq = capi.qparam(a.inp("w", T(wp)), int(wd[0]), int(wd[1]), a.inp("w scale", T(sw)), a.inp("w zero", T(zw)))
        bias = a.inp("bias", T(case["bias"]))
        OH, OW = capi.out_hw(sh)
        oshape = (sh.N, sh.OC, OH, OW)
        n = sh.N * sh.OC * OH * OW
        with capi.knobs(**self.env):
            if self.entry == DIRECT:
                out = a.out("out", oshape, torch.float32)
                info = capi.conv_plan_info(sh, xq, wq, None, out.data_ptr(), 0)
                capi.quantconv2d(xq, wq, bias, sh, out=out, workspace=a.ws("workspace", capi.workspace_bytes(sh, xq.n_bits, wq.n_bits)))
                return Result({"out": out}, _plan_key(info))
            tables = a.ws("tables", int(L.qe_conv_prepared_bytes(ctypes.byref(sh), xq.n_bits, wq.n_bits)))
            capi.check(L.qe_conv_prepare(ctypes.byref(wq), capi._ptr(bias), ctypes.byref(sh), xq.n_bits, *capi._prep(tables),
                                         capi._stream(None)))
            if self.entry == PREPARED:
                out = a.out("out", oshape, torch.float32)
                info = capi.conv_plan_info(sh, xq, wq, None, out.data_ptr(), 0)
                need = int(L.qe_quantconv2d_prepared_workspace_bytes(ctypes.byref(sh), xq.n_bits, wq.n_bits))
                capi.quantconv2d_prepared(xq, wq, bias, sh, tables, out=out, workspace=a.ws("workspace", need))
                return Result({"out": out}, _plan_key(info))
            if self.entry == RESIDUAL_F32:
                identity, status = a.inp("identity", torch.from_numpy(p["identity"])), a.status()
                out = a.out("out", oshape, torch.float32)
                info = capi.conv_plan_info(sh, xq, wq, None, out.data_ptr(), 0)
                capi.quantconv2d_residual_prepared(xq, wq, bias, sh, tables, identity, rq=None, out=out, status=status,
                                                   workspace=a.ws("workspace", capi.residual_workspace_bytes(sh, xq, wq, None)))
                return Result({"out": out, "status": status}, _plan_key(info) + (capi.residual_path(sh, xq, wq, None),))
            sc, zr, qmin, qmax, sign = p["rq"]
            f = lambda v: torch.tensor([v], dtype=torch.float32)
            rq = capi.requant(a.inp("rq scale", f(sc)), a.inp("rq zero", f(zr)), qmin, qmax, 8, sign)
            codes, status = a.out("codes", n, torch.uint8), a.status()
            if self.entry == REQUANT:
                info = capi.conv_plan_info(sh, xq, wq, rq, 0, codes.data_ptr())
                need = int(L.qe_quantconv2d_requant_workspace_bytes(ctypes.byref(sh), ctypes.byref(xq), ctypes.byref(wq), ctypes.byref(rq)))
                capi.quantconv2d_requant_prepared(xq, wq, bias, sh, tables, rq, out=codes, status=status,
                                                  workspace=a.ws("workspace", need))
                return Result({"codes": codes, "status": status}, _plan_key(info) + (capi.requant_path(sh, xq, wq, rq),))
            identity = a.inp("identity", torch.from_numpy(p["identity"]))
            out = a.out("out", oshape, torch.float32)
            info = capi.conv_plan_info(sh, xq, wq, rq, out.data_ptr(), codes.data_ptr())
            need = capi.residual_workspace_bytes(sh, xq, wq, rq)
            capi.quantconv2d_residual_prepared(xq, wq, bias, sh, tables, identity, rq=rq, out=out, codes=codes, status=status,
                                               workspace=a.ws("workspace", need))
            return Result({"out": out, "codes": codes, "status": status}, _plan_key(info) + (capi.residual_path(sh, xq, wq, rq),))

    def check_ref(self, r):
        """conftest.conv_tolerance with the oracle's two fp32 chains on every element; the fused epilogues against the
        float64 value of their own result: codes within the tie band of the float64 codes (test_lin_instances_gpu's rule),
        relu(conv + identity) with one more fp32 rounding (relu does not grow an error)."""
        from test_conv_gpu import _assert_conv_close
        p = self.problem()
        case = p["case"]
        allowed = conv_tolerance(case["o32"], case["o64"], case["o32"], case["fma"])[1]
        if self.entry in (DIRECT, PREPARED):
            _assert_conv_close(r.outs["out"].cpu().numpy(), case["o64"], case["o32"], self.id, case["fma"])
            return
        sc, zr, qmin, qmax, sign = p["rq"]
        sc, zr = float(np.float32(sc)), float(np.float32(zr))
        assert int(r.outs["status"].item()) == 0, self.id
        v, y_err = case["o64"], allowed
        if self.entry in (RESIDUAL, RESIDUAL_F32):
            s = case["o64"] + p["identity"].astype(np.float64)
            v = np.maximum(s, 0.0)
            bound = allowed + EPS24 * (np.abs(s) + allowed)
            _within(r.outs["out"].cpu().numpy(), v, bound, self.id)
            y_err = float(bound.max())
            if self.entry == RESIDUAL_F32:
                return
        cq = tl._stored_to_q(r.outs["codes"].view(v.shape), sign).cpu().numpy()
        tl._check_codes_vs_f64(cq, v, y_err, None, sc, zr, qmin, qmax, self.id)


@functools.lru_cache(maxsize=None)
def _conv_problem(table, i):
    """The operands of a row with the oracle's three evaluations, the consumer's quantiser (test_conv_instances_gpu's:
    amax / 100 clips a few percent, a zero point off zero) and the residual block's identity: once, shared, unchanged."""
    from test_conv_gpu import _random_case
    from test_requant_gpu import _oracle_chains
    if table == "mfma":
        import test_conv_instances_gpu as tci
        case = tci._case(i, 1)
    else:
        import pwr_instances as pi
        shp = pi.ROWS[i][0]
        zeros, has_bias = i % 3 == 1, i % 4 != 3
        case = _random_case(np.random.RandomState(4343 + i), *shp, 8, 1, 8, 0 if zeros else 1, w_pc=True, a_pc=False, zeros=zeros,
                            bias=has_bias)
        case["o32"], case["fma"], case["o64"] = _oracle_chains(case)
    sign = i % 2 == 0
    qmin, qmax = (-128.0, 127.0) if sign else (0.0, 255.0)
    ident = np.random.RandomState(9000 + i).normal(0, float(np.abs(case["o64"]).std()) + 1e-3, size=case["o64"].shape).astype(np.float32)
    sc = max(float(np.abs(case["o64"]).max()) / 100.0, 1e-6)
    zr = ([0.37, -2.0, 5.5] if sign else [-117.25, -3.0, -64.5])[i % 3]
    return dict(case=case, rq=(sc, zr, qmin, qmax, sign), identity=ident)


def _conv_rows():
    """conv_instances rows: for every distinct `expected` the row with the fewest MACs, then -- fewest MACs first -- rows
    until the re-quantising instances conv_instances.covered() counts are reached as well."""
    import conv_instances as ci
    best = {}
    for i, row in enumerate(ci.ROWS):
        if row[4] not in best or _conv_macs(row[0]) < _conv_macs(ci.ROWS[best[row[4]]][0]):
            best[row[4]] = i
    chosen = sorted(best.values())
    reached = set()
    for i in chosen:
        reached |= ci.row_instances(ci.ROWS[i])
    for i in sorted(set(range(len(ci.ROWS))) - set(chosen), key=lambda k: _conv_macs(ci.ROWS[k][0])):
        if ci.covered() <= reached:
            break
        new = ci.row_instances(ci.ROWS[i]) - reached
        if new:
            chosen.append(i)
            reached |= new
    return sorted(chosen)


def conv_cases():
    import conv_instances as ci
    out = []
    for i in _conv_rows():
        row = ci.ROWS[i]
        out += [ConvCase("mfma", i, DIRECT), ConvCase("mfma", i, PREPARED)]
        for env, want_rq, _ in ci.modes(row):
            if want_rq:
                out.append(ConvCase("mfma", i, REQUANT, env=env))
        c = ConvCase("mfma", i, RESIDUAL)
        with capi.knobs(**c.env):
            if capi.residual_path(c._sh(), _qparam_host(c.xb), _qparam_host(c.wb), _rq_host()) == 1:
                out.append(c)
    # no kernel of these routes adds the identity itself (only the resident-tile ones do: pwr_cases); the two-pass route is
    # the workspace case of the residual entry point, so the cheapest row runs it once
    if not any(c.entry == RESIDUAL for c in out):
        out.append(ConvCase("mfma", min(_conv_rows(), key=lambda k: _conv_macs(ci.ROWS[k][0])), RESIDUAL))
    return out


def pwr_cases():
    import pwr_instances as pi
    best = {}
    for i, (shape, base, note, env) in enumerate(pi.ROWS):
        if base not in best or _conv_macs(shape) < _conv_macs(pi.ROWS[best[base]][0]):
            best[base] = i
    out = []
    for i in sorted(best.values()):
        out += [ConvCase("pwr", i, PREPARED), ConvCase("pwr", i, REQUANT)]
        if pi.has_res(pi.ROWS[i][1]):
            out += [ConvCase("pwr", i, RESIDUAL), ConvCase("pwr", i, RESIDUAL_F32)]
    return out


# ---- float-input convolutions ----------------------------------------------------------------------------------------
def _f32_rows():
    import f32_instances as fi
    rows = [fi.rows_of(k)[0] for k in sorted(fi.every_instance())]
    f = fi.FALLBACK[0]
    return rows + [fi.Row(*f[:9], instance=f[10] or "VALU", note="")], f[9]


@functools.lru_cache(maxsize=None)
def _f32_problem(k):
    import test_f32_instances_gpu as tf
    r = _f32_rows()[0][k]
    rng = tf._rng(r, "mem")
    w = tf._weights(r, rng, exact=False)
    x = rng.normal(0, 1, size=(r.N, r.IC, r.H, r.W)).astype(np.float32)
    return dict(r=r, w=w, x=x, o64=tf._oracle(r, x, w, "f64"), o32=tf._oracle(r, x, w, "fp32"), fma=tf._oracle(r, x, w, "fp32_fma"))


class F32ConvCase(Case):
    """qe_quantconv2d_float_input_ws, or qe_conv_f32_prepare + qe_quantconv2d_float_input_prepared, on the first row of an
    instance of tests/f32_instances.py (or the first FALLBACK row: the order-preserving VALU kernel)."""
    family = "conv_f32"

    def __init__(self, k, prepared):
        import f32_instances as fi
        rows, fenv = _f32_rows()
        self.k, self.prepared, self.r = k, prepared, rows[k]
        self.env = dict(fenv or {}) if self.r.instance == "VALU" else {}
        self.fn = "qe_quantconv2d_float_input_prepared" if prepared else "qe_quantconv2d_float_input_ws"
        self.expected = self.r.instance
        self.id = "%s-%s" % (self.fn[3:], fi.row_id(self.r))

    def _kernel(self, sh):
        info = capi.conv_f32_plan_info(sh)
        return capi.F32_KERNELS[info.kernel] if info.ok else "VALU"

    def host(self):
        import f32_instances as fi
        sh = capi.conv_shape(*fi.shape_of(self.r))
        with capi.knobs(**self.env):
            assert self._kernel(sh) == self.expected, self.id
            need = int(capi.lib().qe_quantconv2d_float_input_workspace_bytes(ctypes.byref(sh), 8))
        return {self.expected}, {"qe_quantconv2d_float_input_workspace_bytes": need}

    def run(self, a):
        import f32_instances as fi
        p = _f32_problem(self.k)
        r, w, L = p["r"], p["w"], capi.lib()
        T = lambda v: None if v is None else torch.from_numpy(np.ascontiguousarray(v))
        sh = capi.conv_shape(*fi.shape_of(r))
        x = a.inp("x", T(p["x"]))
        wq = capi.qparam(a.inp("w", T(w["wp"])), w["bits"], w["signed"], a.inp("w scale", T(w["sw"])), a.inp("w zero", T(w["zw"])))
        bias = a.inp("bias", T(w["bias"]))
        OH, OW = capi.out_hw(sh)
        out = a.out("out", (r.N, r.OC, OH, OW), torch.float32)
        with capi.knobs(**self.env):
            kernel = self._kernel(sh)
            ws = a.ws("tables" if self.prepared else "workspace",
                      int(L.qe_quantconv2d_float_input_workspace_bytes(ctypes.byref(sh), wq.n_bits)))
            if self.prepared:
                capi.check(L.qe_conv_f32_prepare(ctypes.byref(wq), capi._ptr(bias), ctypes.byref(sh), *capi._prep(ws), capi._stream(None)))
                capi.check(L.qe_quantconv2d_float_input_prepared(x.data_ptr(), ctypes.byref(wq), capi._ptr(bias), ctypes.byref(sh),
                                                                 *capi._prep(ws), out.data_ptr(), capi._stream(None)))
            else:
                capi.check(L.qe_quantconv2d_float_input_ws(x.data_ptr(), ctypes.byref(wq), capi._ptr(bias), ctypes.byref(sh),
                                                           out.data_ptr(), *capi._prep(ws), capi._stream(None)))
        return Result({"out": out}, kernel)

    def check_ref(self, r):
        from test_conv_gpu import _assert_conv_close
        p = _f32_problem(self.k)
        _assert_conv_close(r.outs["out"].cpu().numpy(), p["o64"], p["o32"], self.id, p["fma"])


def f32_conv_cases():
    return [F32ConvCase(k, prepared) for k in range(len(_f32_rows()[0])) for prepared in (False, True)]


FAMILIES = {"linear": linear_cases, "ew": ew_cases, "attention": attention_cases, "conv": conv_cases, "pwr": pwr_cases,
            "conv_f32": f32_conv_cases}


@functools.lru_cache(maxsize=None)
def cases(family):
    got = FAMILIES[family]()
    ids = [c.id for c in got]
    assert len(set(ids)) == len(ids), sorted(i for i in ids if ids.count(i) > 1)
    return got


def all_cases():
    return [c for f in FAMILIES for c in cases(f)]


# ---- the three calls -------------------------------------------------------------------------------------------------
def run_contract(case, offs=None):
    """Plain call (at the same residues, when offs is given), then the case inside a 0x00 and a 0xFF arena.
    (a) no guard byte and no input changed; (b) every output equals the plain call's as bytes -- and, the two pre-fills
    being opposite, was written; (c) the query names the same kernel for the arena's pointers as for the plain call's, and
    on aligned buffers the kernel the table records.  Returns the plain call's Result (None for a refused case: there all
    three calls raise QeError and no byte of any arena buffer changes)."""
    if case.refused:
        for a in (Plain(offs), Poisoned(arena.FILLS[0], offs), Poisoned(arena.FILLS[1], offs)):
            try:
                case.run(a)
            except capi.QeError:
                if a.fill is not None:
                    a.arena.check("%s (refused), fill 0x%02x" % (case.id, a.fill), refused=True)
                continue
            raise AssertionError("%s: the call was to be refused" % case.id)
        return None
    plain = case.run(Plain(offs))
    torch.cuda.synchronize()
    if offs is None:
        assert case.names_expected(plain.kernel), "%s: runs on %r, the table says %r" % (case.id, plain.kernel, case.expected)
    for fill in arena.FILLS:
        a = Poisoned(fill, offs)
        what = "%s, fill 0x%02x%s" % (case.id, fill, " offsets %s" % offs if offs else "")
        got = case.run(a)
        a.check(what)                                                                           # (a)
        assert got.kernel == plain.kernel, "%s: the query names %r, for plain tensors %r" % (what, got.kernel, plain.kernel)   # (c)
        assert sorted(got.outs) == sorted(plain.outs)
        for name, t in got.outs.items():                                                        # (b)
            same = arena.same_bytes(t, plain.outs[name])
            if not same:
                g, w = (v.contiguous().reshape(-1).view(torch.uint8) for v in (t, plain.outs[name]))
                bad = (g != w).nonzero()
                raise AssertionError("%s: output %r differs from the plain call's in %d of %d bytes, the first at byte %d"
                                     % (what, name, bad.numel(), g.numel(), int(bad[0])))
    return plain
