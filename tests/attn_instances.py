"""One case per instance of the two attention kernels (qe_attention.hip): attn_mfma_kernel<D, MODE>, D = 16 .. 128 in
steps of 16 and 14 operand modes, and attn_valu_kernel<NO, MODE>, NO = ceil(d / 64) = 1 .. 4 and 8 operand modes.

Each ROWS entry is (kernel, d, S, has_mask, has_bias, causal, mask_kind) at N = 2, H = 2, L = 40: two query tiles, the
second ragged, and two key tiles, the second ragged, with S != L.  S = 44 takes the 16-byte mask loads (kVec4): the last
tile's runs of four that start at keys 32, 36 and 40 are valid, those from 44 on must be dropped whole; S = 45 takes the
scalar loads.  The operands of a row (operands()):
  mask   additive2d (L, S) or holes3d (N*H, L, S), alternating over the table; a holes3d row keeps a key visible that
         the row's other operands leave visible too;
  bias   pad_front, which blanks the whole first key tile of every image -- except under causal, where query t < f_n would
         keep no key at all (a NaN row, and an element left out of the comparison): there the bias is pad_mid, which
         keeps keys [0, a_n), a_n <= 7, and blanks the rest of the first tile.  No key bias can blank a whole first tile
         under causal (query 0 sees key 0 only), so no causal row of the table meets a tile with no visible key;
  causal the kernel's own flag.
So every row keeps a visible key in every query row and every output element is compared.

instance() restates only attn_run's dispatch: which template instance a call lands on once qe_attention_masked_path has
chosen the kernel."""
import numpy as np

import attention_ref as ar
import test_attention_gpu as base

MFMA, VALU = "attn_mfma_kernel", "attn_valu_kernel"
kMask, kBias, kCausal, kVec4 = 1, 2, 4, 8
N, H, L = 2, 2, 40
S_VEC4, S_SCALAR = 44, 45
MFMA_D = tuple(range(16, 129, 16))
VALU_D = {1: 20, 2: 72, 3: 136, 4: 256}
COMBOS = [(m, b, c) for c in (False, True) for b in (False, True) for m in (False, True)]


def instance(kernel, d, S, has_mask, has_bias, causal, mask_sn=0, mask_sh=0):
    """(attn_mfma_kernel, D, MODE) or (attn_valu_kernel, ceil(d / 64), MODE & ~kVec4): MODE is kMask | kBias | kCausal by
    the operands present, plus kVec4 iff a mask or a bias exists, S % 4 == 0 and both mask strides are multiples of 4."""
    mode = (kMask if has_mask else 0) | (kBias if has_bias else 0) | (kCausal if causal else 0)
    if (has_mask or has_bias) and S % 4 == 0 and mask_sn % 4 == 0 and mask_sh % 4 == 0:
        mode |= kVec4
    if kernel == MFMA:
        assert d in MFMA_D
        return (MFMA, d, mode)
    assert kernel == VALU and 0 < d <= 256
    return (VALU, -(-d // 64), mode & ~kVec4)


def kernel_name(inst):
    """As a kernel trace shows it (inside `void qe::...(qe::AttnArgs)`)."""
    return "%s<%d, %d>" % inst


def dispatchable():
    """Every instance attn_run can launch: 8 x 14 attn_mfma_kernel and 4 x 8 attn_valu_kernel."""
    modes = [m | b | c for c in (0, kCausal) for b in (0, kBias) for m in (0, kMask)]
    out = {(VALU, no, mode) for no in (1, 2, 3, 4) for mode in modes}
    for D in MFMA_D:
        out |= {(MFMA, D, mode) for mode in modes}
        out |= {(MFMA, D, mode | kVec4) for mode in modes if mode & (kMask | kBias)}
    return out


def mask_strides(mask_kind, S):
    """(mask_sn, mask_sh) as capi.attention passes them for a row's mask."""
    return (H * L * S, L * S) if mask_kind == "holes3d" else (0, 0)


def _rows():
    rows = []
    for kernel, sizes in ((MFMA, [(D // 16, D) for D in MFMA_D]), (VALU, sorted(VALU_D.items()))):
        for idx, d in sizes:
            for m, b, c in COMBOS:
                kind = ("holes3d" if (idx + b + c) % 2 == 0 else "additive2d") if m else None
                # the VALU kernel has no 16-byte form: one S per mode; neither has one without a mask or a bias
                for S in ((S_VEC4, S_SCALAR) if kernel == MFMA and (m or b) else (S_SCALAR,)):
                    rows.append((kernel, d, S, m, b, c, kind))
    return rows


ROWS = _rows()


def row_instance(row):
    kernel, d, S, m, b, c, kind = row
    return instance(kernel, d, S, m, b, c, *mask_strides(kind, S))


def row_id(row):
    kernel, d, S, m, b, c, kind = row
    return "%s d%d S%d %s" % (kernel_name(row_instance(row)), d, S,
                              "+".join(([kind] if m else []) + (["bias"] if b else []) + (["causal"] if c else [])) or "plain")


def covered():
    """The instances ROWS reaches."""
    return {row_instance(r) for r in ROWS}


def rows_of(kernel, size):
    """The rows of one (kernel, D or NO)."""
    return [r for r in ROWS if row_instance(r)[:2] == (kernel, size)]


def operands(row, seed=0):
    """dict(mask=, key_bias=, causal=) of host arrays for a row (only the operands it has)."""
    kernel, d, S, m, b, c, kind = row
    rng = np.random.RandomState(1000 * d + 10 * S + 4 * c + 2 * b + m + seed)
    ops = {}
    if b:
        ops["key_bias"] = ar.pad_mid(N, S, rng) if c else ar.pad_front(N, S, rng)
    if c:
        ops["causal"] = True
    if m and kind == "additive2d":
        ops["mask"] = ar.additive2d(L, S, rng)
    elif m:
        # keep one key the other operands leave visible: under causal key <= t (key 0 where a bias is present too, which
        # pad_mid never hides), else a key the bias does not pad
        t = np.broadcast_to(np.arange(L)[None, :], (N * H, L))
        if c:
            keep = np.zeros((N * H, L), np.int64) if b else rng.randint(0, 1 << 30, size=(N * H, L)) % (np.minimum(t, S - 1) + 1)
        elif b:
            lo = np.isfinite(ops["key_bias"]).argmax(-1)                            # pad_front: visible keys are [f_n, S)
            keep = np.repeat(lo, H)[:, None] + rng.randint(0, 1 << 30, size=(N * H, L)) % np.repeat(S - lo, H)[:, None]
        else:
            keep = None
        ops["mask"] = ar.holes3d(N, H, L, S, rng, keep=keep)
    return ops


def peaky_operands(S):
    """The three masked cases of the peaky regime (q / k with one score of 60 in the last key tile and one of 58 in the
    first): every additive value is <= 0, so no score rises above the unmasked regime's."""
    al = np.ascontiguousarray(np.broadcast_to(ar.alibi(H, L, S), (N, H, L, S)))
    return {"alibi": dict(mask=al), "pad_front": dict(key_bias=ar.pad_front(N, S, np.random.RandomState(S))),
            "causal+alibi": dict(mask=al, causal=True)}


def peaky_inputs(d, S, peak=60.0):
    """test_attention_gpu's peaky q / k / v (each query row scores 60 on a key of the last key tile and 58 on one of the
    first) with |score| <= peak enforced: at small d the untargeted keys' scores spread with sigma ~ 60 sqrt(2 / d) and some
    pass 100, so a query row whose largest |score| exceeds 60 is scaled down to it; then every row by peak / 60."""
    q, k, v = base._inputs(N, L, S, H, d, "peaky", seed=d + S)
    s = np.einsum("nlhd,nshd->nlhs", q.astype(np.float64), k.astype(np.float64)) * d ** -0.5
    shrink = np.minimum(1.0, 60.0 / np.abs(s).max(-1)) * (peak / 60.0)
    return (q * shrink[..., None]).astype(np.float32), k, v
