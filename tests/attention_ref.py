"""The float64 yardstick of masked attention and the mask generators of tests/test_attention_mask_{cpu,gpu}.py and
tests/test_attn_instances_{cpu,gpu}.py.

ref64(q, k, v, mask, key_bias, causal): softmax_s(scale q.k + mask[n, h, t, s] + key_bias[n, s] [s <= t only]) v in float64
on (N, T, H, d) arrays.  A row with no visible key is NaN (-inf - -inf in the max subtraction), as torch.softmax gives.
Masks are additive float32 arrays (finite or -inf); every generator but `blank_rows` asserts that each row keeps a
visible key, so no element has to be left out of a comparison."""
import numpy as np

NEG = -np.inf


def expand_mask(mask, N, H, L, S):
    """An additive mask of shape (L, S), (N, L, S), (N*H, L, S) or (N, H, L, S) as a (N, H, L, S) view."""
    if mask.shape == (L, S):
        return np.broadcast_to(mask, (N, H, L, S))
    if mask.shape == (N * H, L, S) or mask.shape == (N, H, L, S):
        return mask.reshape(N, H, L, S)
    if mask.shape == (N, L, S):
        return np.broadcast_to(mask[:, None], (N, H, L, S))
    raise ValueError(mask.shape)


def merged(N, H, L, S, mask=None, key_bias=None, causal=False):
    """The one additive (N, H, L, S) float32 array the three operands amount to (what torch's SDPA is given)."""
    m = np.zeros((N, H, L, S), np.float32)
    if mask is not None:
        m = m + expand_mask(mask, N, H, L, S)
    if key_bias is not None:
        m = m + key_bias[:, None, None, :]
    if causal:
        m = m + tril_inf(L, S)
    return m.astype(np.float32)


def visible(m):
    """Per row: does at least one key stay visible?"""
    return np.isfinite(m).any(-1)


def ref64(q, k, v, mask=None, key_bias=None, causal=False, scale=None):
    N, L, H, d = q.shape
    S = k.shape[1]
    q64, k64, v64 = (a.astype(np.float64) for a in (q, k, v))
    s = np.einsum("nlhd,nshd->nhls", q64, k64) * (d ** -0.5 if scale is None else scale)
    s = s + merged(N, H, L, S, mask, key_bias, causal).astype(np.float64)
    with np.errstate(invalid="ignore"):
        s = s - s.max(-1, keepdims=True)
        p = np.exp(s)
        p = p / p.sum(-1, keepdims=True)
        return np.einsum("nhls,nshd->nlhd", p, v64)


# ---- mask generators (float32, additive) ----
def additive2d(L, S, rng):
    """(L, S): finite N(0, 2) values, shared by every image and head.  No tile boundary of its own: it puts a different
    non-zero value under every key of every run of four a lane loads."""
    return rng.normal(0, 2, size=(L, S)).astype(np.float32)


def tril_inf(L, S):
    """Top-left aligned causal mask: key s visible to query t iff s <= t (torch.ones(L, S).tril()).  The diagonal crosses
    every 32-key tile at a different key per row; the tiles above it are the ones a causal wave never visits."""
    m = np.zeros((L, S), np.float32)
    m[np.arange(S)[None, :] > np.arange(L)[:, None]] = NEG
    return m


def holes3d(N, H, L, S, rng, p=0.5, keep=None):
    """(N*H, L, S): random finite values with -inf holes; one key per row is kept visible (a random one, or keep[n*H + h, t]
    where another operand hides keys too).  Holes fall inside the runs of four keys a lane loads and on either side of
    every 32-key tile boundary."""
    m = rng.normal(0, 1, size=(N * H, L, S)).astype(np.float32)
    m[rng.uniform(size=m.shape) < p] = NEG
    if keep is None:
        keep = rng.randint(0, S, size=(N * H, L))
    np.put_along_axis(m, keep[..., None], 0.0, axis=-1)
    assert visible(m).all()
    return m


def pad_tail(N, S, rng):
    """Key bias (N, S): image n keeps its first len_n >= 1 keys (image 0: S - 3, so its cut lies in the last, ragged key
    tile; the others anywhere, whole trailing tiles included)."""
    lengths = rng.randint(1, S + 1, size=N)
    lengths[0] = max(1, S - 3)
    b = np.zeros((N, S), np.float32)
    b[np.arange(S)[None, :] >= lengths[:, None]] = NEG
    assert visible(b).all()
    return b


def pad_front(N, S, rng):
    """Key bias (N, S): image n ignores its first f_n keys; for S > 32, f_n >= 32 blanks the whole first 32-key tile
    (33 .. S - 1 keys, image 0 exactly 32), so a row's running max is still -inf when the first visible key arrives."""
    if S > 32:
        front = rng.randint(32, S, size=N)
        front[0] = 32
    else:
        front = rng.randint(1, S, size=N) if S > 1 else np.zeros(N, np.int64)
    b = np.zeros((N, S), np.float32)
    b[np.arange(S)[None, :] < front[:, None]] = NEG
    assert visible(b).all()
    return b


def pad_mid(N, S, rng):
    """Key bias (N, S) that a causal row survives: image n ignores keys [a_n, b_n), a_n odd in 1 .. 7 and b_n odd in
    33 .. S - 1 (S > 34).  Key 0 stays visible to query 0 (pad_front would leave every causal row t < f_n without a key), the
    rest of the first 32-key tile is blank, the band ends inside the second tile, and both edges fall inside a run of four."""
    assert S > 34
    a = 1 + 2 * rng.randint(0, 4, size=N)
    b = 33 + 2 * rng.randint(0, (S - 34) // 2 + 1, size=N)
    bias = np.zeros((N, S), np.float32)
    s = np.arange(S)[None, :]
    bias[(s >= a[:, None]) & (s < b[:, None])] = NEG
    assert visible(bias).all() and np.isfinite(bias[:, 0]).all() and np.isfinite(bias[:, -1]).all()
    return bias


def alibi(H, L, S):
    """(H, L, S) finite (pass it broadcast to (N, H, L, S)): -slope_h |t - s| with slope_h = 30 / max|t - s| / 2^h,
    largest magnitude 30 (head 0).  Against inputs whose row maximum sits in the last key tile it moves the maximum of the
    early query rows to the first tile, so the online softmax's running max is set early and the late peak arrives as a
    small term, the reverse of the unmasked order; no tile boundary of its own."""
    dist = np.abs(np.arange(L)[:, None] - np.arange(S)[None, :]).astype(np.float64)
    slope = 30.0 / dist.max() / 2.0 ** np.arange(H)
    return (-slope[:, None, None] * dist[None]).astype(np.float32)


def blank_rows(N, H, L, S, rows, rng):
    """(N*H, L, S) finite random mask whose listed (n, h, t) rows are entirely -inf: the declared NaN rows."""
    m = rng.normal(0, 1, size=(N, H, L, S)).astype(np.float32)
    for (n, h, t) in rows:
        m[n, h, t, :] = NEG
    return m.reshape(N * H, L, S)
