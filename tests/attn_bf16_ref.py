"""Yardsticks of the bf16 attention core (qe_attention_bf16), shared by tests/test_attention_bf16_{cpu,gpu}.py and
tests/test_packed_vit_attention_bf16_gpu.py.

The contract (include/quant_engine.h): q^ = bf16(fp32(q scale)), k^ = bf16(k), v^ = bf16(v), round to nearest even; fp32
scores of exact bf16 products plus the fp32 mask / bias; fp32 online softmax; p rounded to bf16 only as the operand of P.V; l
the fp32 sum of the unrounded p; fp32 O and one division.  Against float64 attention on q^, k^, v^ (scale 1) the only error
that is not fp32-level is the rounding of p, relative 2^-8 per element: |out - ref| <= (2^-8 + 1e-5) max|v^| (bound()).

rounded()    the three rounded inputs, built on the host as the kernel builds them
ref64()      attention_ref.ref64 on them, scale 1
emulate()    the contract in numpy: 32-key tiles, online softmax in float32, p through torch.bfloat16
wave_tile()  one wave's two products LANE BY LANE: the fragments as attn_bf16_kernel indexes them, fed to
             v_mfma_f32_32x32x16_bf16's operand layout (A[i][k] and B[k][j] on lane i or j + 32 (k >> 3), element k & 7;
             C[i][j] on lane j + 32 ((i >> 2) & 1), register (i & 3) + 4 (i >> 3)): the check of the two lane maps"""
import numpy as np
import torch

import attention_ref as ar

LOG2E = np.float32(1.4426950408889634)
CASES = [(2, 197, 197, 12, 64), (1, 50, 50, 12, 64), (2, 257, 257, 16, 80), (3, 17, 17, 4, 16), (2, 1, 1, 2, 64),
         (2, 33, 65, 3, 32), (1, 197, 197, 1, 128), (1, 300, 300, 2, 64)]
EXACT_D = (16, 48, 64, 128)
EXACT_LS = ((40, 44), (40, 45), (77, 77))


def bf16(a):
    """Round a float32 array to bf16 (nearest even), returned as float32."""
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(torch.bfloat16).to(torch.float32).numpy()


def rounded(q, k, v, scale=None):
    d = q.shape[-1]
    scale = np.float32(d ** -0.5 if scale is None else scale)
    return bf16(q.astype(np.float32) * scale), bf16(k), bf16(v)


def ref64(qh, kh, vh, **ops):
    return ar.ref64(qh, kh, vh, scale=1.0, **ops)


def bound(vh):
    return (2.0 ** -8 + 1e-5) * float(np.abs(vh).max())


def emulate(qh, kh, vh, mask=None, key_bias=None, causal=False):
    """The contract on rounded (N, T, H, d) inputs, tile by tile; float32 result (N, L, H, d)."""
    N, L, H, d = qh.shape
    S = kh.shape[1]
    s = np.einsum("nlhd,nshd->nhls", qh.astype(np.float64), kh.astype(np.float64)).astype(np.float32)
    add = ar.merged(N, H, L, S, mask, key_bias, False)                # mask + bias first, in fp32
    s = (s + add).astype(np.float32)
    if causal:
        s[..., np.arange(S)[None, :] > np.arange(L)[:, None]] = -np.inf
    v64 = vh.astype(np.float64).transpose(0, 2, 1, 3)                  # (N, H, S, d)
    m = np.full((N, H, L), -np.inf, np.float32)
    l = np.zeros((N, H, L), np.float32)
    o = np.zeros((N, H, L, d), np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for k0 in range(0, S, 32):
            st = s[..., k0:k0 + 32]
            mn = np.maximum(m, st.max(-1))
            empty = mn == -np.inf
            alpha = np.where(empty, np.float32(1), np.exp2(((m - mn) * LOG2E).astype(np.float32))).astype(np.float32)
            msub = np.where(empty, np.float32(0), mn).astype(np.float32)
            p = np.exp2(((st - msub[..., None]) * LOG2E).astype(np.float32)).astype(np.float32)
            l = (l * alpha + p.sum(-1, dtype=np.float32)).astype(np.float32)
            pv = np.einsum("nhls,nhsd->nhld", bf16(p).astype(np.float64), v64[:, :, k0:k0 + 32])
            o = (o * alpha[..., None] + pv).astype(np.float32)
            m = mn
        return (o / l[..., None]).astype(np.float32).transpose(0, 2, 1, 3)


def exact_case(d, L, S, bias=False, seed=0, N=2, H=2):
    """q = 0, k random, v integers in [-8, 8], a 0 / -inf hole mask (attention_ref.holes3d's pattern): every visible p is
    exactly 1, l the visible count, O the integer sum.  (q, k, v, ops, expected float32 (N, L, H, d))."""
    rng = np.random.RandomState(100 * d + L + S + seed)
    q = np.zeros((N, L, H, d), np.float32)
    k = rng.normal(0, 1, size=(N, S, H, d)).astype(np.float32)
    v = rng.randint(-8, 9, size=(N, S, H, d)).astype(np.float32)
    ops = {}
    keep = None
    if bias:
        ops["key_bias"] = ar.pad_front(N, S, rng)
        lo = np.isfinite(ops["key_bias"]).argmax(-1)                   # visible keys are [f_n, S)
        keep = np.repeat(lo, H)[:, None] + rng.randint(0, 1 << 30, size=(N * H, L)) % np.repeat(S - lo, H)[:, None]
    holes = ar.holes3d(N, H, L, S, rng, keep=keep)
    ops["mask"] = np.where(np.isfinite(holes), np.float32(0), np.float32(-np.inf)).astype(np.float32)
    vis = np.isfinite(ar.merged(N, H, L, S, **ops))                    # (N, H, L, S)
    assert vis.any(-1).all()
    total = np.einsum("nhls,nshd->nlhd", vis.astype(np.float64), v.astype(np.float64))
    count = vis.sum(-1).transpose(0, 2, 1)[..., None]                  # (N, L, H, 1)
    return q, k, v, ops, total.astype(np.float32) / count.astype(np.float32)


# ---- one wave, lane by lane ----
def _mfma_32x32x16(A, B, C):
    """A, B: (64, 8) fragments, C: (64, 16) accumulator registers -> the new accumulator (float64 arithmetic)."""
    lane = np.arange(64)
    a = np.zeros((32, 16))
    b = np.zeros((16, 32))
    for j in range(8):
        a[lane & 31, 8 * (lane >> 5) + j] = A[:, j]
        b[8 * (lane >> 5) + j, lane & 31] = B[:, j]
    c = a @ b
    out = C.astype(np.float64).copy()
    for r in range(16):
        out[:, r] += c[(r & 3) + 8 * (r >> 2) + 4 * (lane >> 5), lane & 31]
    return out


def wave_tile(q, k, v, p):
    """One wave, one 32-key tile at head size D: q, k, v (32, D), p (32 queries, 32 keys).  Returns (S^T as the score
    accumulator's registers decode it: (32 queries, 32 keys); O = P V (32 queries, D)), both through the kernel's fragments."""
    D = q.shape[1]
    HALF, KS, NB = D // 2, D // 16, (D + 31) // 32
    lane = np.arange(64)
    lo, hi = lane & 31, lane >> 5
    sc = np.zeros((64, 16))
    for s in range(KS):
        dims = hi[:, None] * HALF + 8 * s + np.arange(8)[None, :]
        sc = _mfma_32x32x16(k[lo[:, None], dims], q[lo[:, None], dims], sc)
    crow = lambda r: (r & 3) + 8 * (r >> 2) + 4 * hi                  # key of register r on each lane
    scores = np.zeros((32, 32))
    for r in range(16):
        scores[lo, crow(r)] = sc[:, r]
    # P^T operand: register r of the accumulator holds p[query lo][key crow(r)]
    pr = np.stack([p[lo, crow(r)] for r in range(16)], axis=1)        # (64, 16)
    out = np.zeros((32, D))
    for b in range(NB):
        o = np.zeros((64, 16))
        for s in range(2):
            vf = np.zeros((64, 8))
            for j in range(8):
                c = 32 * b + lo
                vf[:, j] = np.where(c < D, v[crow(8 * s + j), np.minimum(c, D - 1)], 0.0)
            o = _mfma_32x32x16(vf, pr[:, 8 * s:8 * s + 8], o)
        for r in range(16):                                           # O^T row (column of out) crow(r), query on the lane
            c = 32 * b + crow(r)
            ok = c < D
            out[lo[ok], c[ok]] = o[ok, r]
    return scores, out
