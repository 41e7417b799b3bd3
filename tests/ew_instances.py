"""The elementwise kernel family and the cases that take each instance to its edges, shared by tests/test_ew_instances_cpu.py
(coverage, and the discriminating power of the inputs) and the GPU tests tests/test_ew_instances_gpu.py,
test_ew_instances_gridcap_gpu.py and test_ew_instances_pool_gpu.py.

Instances (93):
  ("tpack_kernel", T, bits, QM)   qe_tpack.hip: QM 0 = qe_tpack for the 8 element types, QM 1 / 2 = qe_quantize_pack per tensor /
                                  per channel (float32 only): 64 + 16
  ("tunpack_kernel", bits)        qe_tunpack: 8
  ("act_quant_kernel", act)       qe_quantize_pack_act with an fp32 output or a GELU: 2
  ("patchify_quant_kernel",), ("maxpool2d_codes_kernel",), ("global_avgpool_kernel",)

What the GPU tests hold every case to: codes are the fp32 operation sequence of ew_ref.quantise bit for bit, no byte
outside the output changes (`Guarded`), and the range flag is raised from any position."""
import numpy as np

import ew_ref

TILE = 8192               # elements per tpack / tunpack tile (TP_TILE)
TP_MAX_BLOCKS = 2048      # tiles past this many go round the grid-stride loop (kNumCU * 8)
DTYPES = ("uint8", "int8", "int16", "int32", "int64", "float16", "float32", "float64")
ITEMSIZE = {"uint8": 1, "int8": 1, "int16": 2, "int32": 4, "int64": 8, "float16": 2, "float32": 4, "float64": 8}
PAIRS = [(b, s) for b in range(1, 9) for s in (False, True)]
NS = (1, 7, 31, 32, 33, 8191, 8192, 8193, 3 * 8192 + 5)


def in_offset(dtype):
    """An element offset that breaks the min(16, 4 * sizeof(T)) alignment of the vector loads: odd for 1-, 2- and 4-byte
    types, 1 for 8-byte types (8-byte aligned, not 16)."""
    return 1 if ITEMSIZE[dtype] == 8 else 3


OUT_OFFSET = 5            # bytes; not a multiple of 16
# (input offset in elements or None = in_offset(dtype), output offset in bytes): aligned, input off, output off
TPACK_VARIANTS = ((0, 0), (None, 0), (0, OUT_OFFSET))
F32_CROSS_BITS = (3, 8)
F32_CROSS = [(i, o) for i in (0, 1, 2, 3) for o in (0, 1, 8, 15)]


def tpack_values(dtype, bits, sign):
    """(lowest, highest) value a tpack case draws: the width's code range cut to what the element type holds."""
    lo, hi = ew_ref.qrange(bits, sign)
    if dtype == "uint8":
        lo = max(lo, 0)
    if dtype == "int8":
        hi = min(hi, 127)
    return lo, hi


TPACK_CASES = [(t, b, s) for t in DTYPES for (b, s) in PAIRS]

# ---- quantisers ----------------------------------------------------------------------------------------------------
# per-tensor (scale, zero): each separates the reciprocal-multiply and the float64 variants on tie-dense inputs (the CPU
# test measures it).  (0.61, 1.5), which test_quantize_pack_gpu.py's round trip uses, does NOT separate the reciprocal.
PER_TENSOR = ((0.37, -1.25), (1.7, 0.0), (0.013, 3.0))
REJECTED = ((0.61, 1.5),)
INNERS = (1, 2, 3, 4, 5, 49, 196, 1023, 8192, 8193, 12544)
CHANNELS = (2, 3, 64)
PC_MAX_N = 7 * TILE + 5   # per-channel cases stop here: C = 2 and 3 wrap at every inner, C = 64 up to inner = 880


def channel_params(n_ch):
    """Per-channel (scale, zero) of a case with n_ch channels."""
    rng = np.random.RandomState(7000 + n_ch)
    return rng.uniform(0.05, 2.0, size=n_ch).astype(np.float32), rng.uniform(-3.0, 3.0, size=n_ch).astype(np.float32)


def tensor_params(i):
    s, z = PER_TENSOR[i % len(PER_TENSOR)]
    return np.array([s], np.float32), np.array([z], np.float32)


def scale_sets():
    """Every (name, scale, zero, inner) the GPU tests quantise with; inner = 1 puts neighbouring elements on different
    channels, which is the hardest mix for a per-set measurement."""
    out = [("tensor %g, %g" % sz, np.array([sz[0]], np.float32), np.array([sz[1]], np.float32), 1) for sz in PER_TENSOR]
    out += [("%d channels" % c,) + channel_params(c) + (1,) for c in CHANNELS]
    return out


def pc_n(inner, n_ch):
    """Elements of a per-channel case: one wrap of the channels and a ragged bit more, at least two tiles."""
    return min(max(inner * n_ch + inner + 5, 2 * TILE + 5), PC_MAX_N)


QPACK_PC_CASES = [(inner, c) for inner in INNERS for c in CHANNELS]
QPACK_OFFSETS = ((1, 0), (2, 0), (3, 0), (0, 1), (0, 8), (0, 15), (3, 5))   # (x offset in floats, out offset in bytes)

# qe_quantize_pack_act: (act, y) with y None | "new" | "inplace"; (None, None) is qe_quantize_pack itself
ACT_MODES = ((None, "new"), (None, "inplace"), ("gelu", None), ("gelu", "new"), ("gelu", "inplace"))
ACT_NS = tuple(4096 + r for r in range(8)) + (1, 7, 9)
ACT_FLOAT_OFFSETS = (0, 1, 2, 3)
ACT_CODE_OFFSETS = (0, 4, 8, 1)   # at 8 bits: 0 and 8 take the 8-byte store, 4 and 1 the byte loop
ACT_OFFSET_N = 4099


def flag_positions(n, epl):
    """Where the range-flag tests put the one offending element, for an n with a ragged tail past at least one whole tile:
    name -> index.  epl: consecutive elements a lane owns (tpack: 16 / 8 / 4 for 1- / 2- / wider-byte types; 8 for the
    kernels that work in groups of 8)."""
    assert n > TILE and n % TILE != 0 and n % 8 != 0
    return {"element 0": 0, "last element, in the ragged tail": n - 1, "last element of tile 0": TILE - 1,
            "first element of the ragged tile": TILE, "lane 63 of wave 0": 63 * epl + 1,
            "lane 63 of the last wave": 255 * epl + epl - 1}


def tpack_epl(dtype):
    return {1: 16, 2: 8}.get(ITEMSIZE[dtype], 4)


FLAG_N = TILE + 1029      # one whole tile and a ragged one; 1029 % 8 = 5

# ---- past the grid caps --------------------------------------------------------------------------------------------
GRIDCAP_N = (TP_MAX_BLOCKS + 1) * TILE + 5      # > 2048 tiles, and > 8192 * 256 groups of 8 (the act / residual grid cap)
GRIDCAP_PATCHIFY = (112, 3, 224, 224, 16)       # 16 859 136 elements: more groups of 8 than kNumCU * 32 blocks of 256 hold
PATCHIFY_MAX_GROUPS = 256 * 32 * 256


def gridcap_windows(n):
    """(start, count) of the windows compared with ew_ref: the first two tiles, the tiles either side of tile 2048, the last
    whole tile with the ragged one.  Starts are multiples of 8, so a window begins on a byte at every width."""
    last = (n - (TILE + 5)) // 8 * 8
    return ((0, 2 * TILE), ((TP_MAX_BLOCKS - 1) * TILE, 2 * TILE), (last, n - last))


# ---- quantize_patchify: (N, C, H, W, p, x offset in floats, note) ----------------------------------------------------
PATCHIFY_CASES = [
    (2, 3, 32, 32, 16, 0, "p % 8 == 0: the two 16-byte loads"),
    (2, 3, 28, 28, 14, 0, "p % 8 != 0: the scalar gather"),
    (3, 3, 16, 24, 8, 1, "p % 8 == 0 with x off by one float: the scalar gather"),
    (1, 3, 6, 9, 3, 0, "162 elements: a ragged last group of 2"),
    (5, 1, 5, 5, 5, 2, "125 elements: a ragged last group of 5, x off by two floats"),
    (9, 4, 48, 32, 16, 0, "several blocks"),
]
PATCHIFY_BITS = ((8, True), (8, False), (4, True), (3, False))

# ---- maxpool2d_codes: (N, C, H, W, kernel, stride, padding, note) ----------------------------------------------------
MAXPOOL_CASES = [
    (1, 41, 2, 2, 3, 2, 1, "OH*OW = 1, k > H with padding: a thread walks 16 planes"),
    (5, 9, 2, 2, 3, 1, 1, "OH*OW = 4, k > H with padding"),
    (1, 41, 6, 6, 2, 2, 0, "OH*OW = 9, n_out % 16 = 1"),
    (7, 7, 5, 9, 3, 2, 1, "OH*OW = 15, n_out % 16 = 15"),
    (1, 7, 3, 19, 3, 1, 0, "OH*OW = 17"),
    (5, 8, 8, 11, 2, 3, 0, "stride > k, OH*OW = 12"),
    (2, 8, 18, 18, 3, 2, 1, "the stem's pool, small"),
    (3, 16, 33, 33, 3, 2, 1, "several blocks, odd planes"),
]
MAXPOOL_OUT_OFFSETS = (0, 1, 8)


def maxpool_out_hw(H, W, k, s, p):
    return (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1


# ---- global_avgpool -------------------------------------------------------------------------------------------------
AVGPOOL_P = (1, 2, 3, 5, 49, 239, 240)
AVGPOOL_P_REFUSED = 241
AVGPOOL_PLANES = (1, 63, 64, 65, 185)
AVGPOOL_OFFSETS = (0, 1, 2, 3)


# ---- coverage --------------------------------------------------------------------------------------------------------
def every_instance():
    out = {("tpack_kernel", t, b, 0) for t in DTYPES for b in range(1, 9)}
    out |= {("tpack_kernel", "float32", b, qm) for b in range(1, 9) for qm in (1, 2)}
    out |= {("tunpack_kernel", b) for b in range(1, 9)}
    out |= {("act_quant_kernel", "none"), ("act_quant_kernel", "gelu")}
    out |= {("patchify_quant_kernel",), ("maxpool2d_codes_kernel",), ("global_avgpool_kernel",)}
    return out


def tpack_instances(case):
    t, b, _ = case
    return {("tpack_kernel", t, b, 0), ("tunpack_kernel", b)}     # every tpack case unpacks a stream of its width too


def qpack_instances(pair):
    """A (bits, sign) pair of the quantize_pack tests runs PER_TENSOR (QM 1) and QPACK_PC_CASES (QM 2)."""
    return {("tpack_kernel", "float32", pair[0], 1), ("tpack_kernel", "float32", pair[0], 2)}


def act_instances(mode):
    return {("act_quant_kernel", "gelu" if mode[0] == "gelu" else "none")}


def covered():
    out = set()
    for c in TPACK_CASES:
        out |= tpack_instances(c)
    for p in PAIRS:
        out |= qpack_instances(p)
    for m in ACT_MODES:
        out |= act_instances(m)
    if PATCHIFY_CASES:
        out.add(("patchify_quant_kernel",))
    if MAXPOOL_CASES:
        out.add(("maxpool2d_codes_kernel",))
    if AVGPOOL_P and AVGPOOL_PLANES:
        out.add(("global_avgpool_kernel",))
    return out


# ---- guard bands -----------------------------------------------------------------------------------------------------
FILL = 0xA5
BAND = 64                 # bytes in front of and behind every output; a multiple of 16, so `offset` alone sets the alignment


class Guarded:
    """An output of `nbytes` bytes at byte `offset` past a 16-byte boundary, inside a buffer prefilled with 0xA5.  The
    kernel writes to `.out` (a uint8 view; `.view(dtype)` for typed outputs); `.result()` brings the buffer back once,
    asserts that no byte in front of or behind the output changed, and returns the output's bytes as numpy.  The prefill
    is a pattern and not zeros so that a byte the kernel never wrote differs from the reference."""

    def __init__(self, nbytes, offset=0, device="cuda:0"):
        import torch
        self.nbytes, self.lead = int(nbytes), BAND + int(offset)
        self.buf = torch.full((self.lead + self.nbytes + BAND + 16,), FILL, dtype=torch.uint8, device=device)
        assert self.buf.data_ptr() % 16 == 0
        self.out = self.buf[self.lead:self.lead + self.nbytes]

    def view(self, dtype):
        return self.out.view(dtype)

    def result(self, what=""):
        b = self.buf.cpu().numpy()
        front, back = b[:self.lead], b[self.lead + self.nbytes:]
        assert (front == FILL).all(), "%s: wrote %d bytes in front of the output (first at %d)" % (
            what, int((front != FILL).sum()), int(np.flatnonzero(front != FILL)[0]) - self.lead)
        assert (back == FILL).all(), "%s: wrote %d bytes behind the output (first at +%d)" % (
            what, int((back != FILL).sum()), int(np.flatnonzero(back != FILL)[0]))
        return b[self.lead:self.lead + self.nbytes]


def device_input(values, dtype, offset=0, device="cuda:0"):
    """`values` (numpy) as a contiguous device tensor of `dtype` that starts `offset` elements into its allocation."""
    import torch
    t = torch.from_numpy(np.array(values)).to(getattr(torch, dtype) if isinstance(dtype, str) else dtype)
    base = torch.zeros(t.numel() + offset + 8, dtype=t.dtype, device=device)
    assert base.data_ptr() % 16 == 0
    base[offset:offset + t.numel()] = t.to(device)
    return base[offset:offset + t.numel()]
