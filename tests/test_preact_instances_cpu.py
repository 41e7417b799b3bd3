"""CPU: the instance table of qe_affine_relu_quantize_pack against the host-side plan, and tests/preact_ref.py against the
reference's own BatchNorm2d -> ReLU -> Quantizer chain (G14 (a)) and against the two nearly-right evaluations of the contract."""
import numpy as np
import pytest

import preact_instances as pi
import preact_ref
from conftest import Golden
from quantize_amd import capi


@pytest.fixture(scope="module")
def g14():
    return Golden("g14_wrn.npz")


def test_symbols_and_instance_names():
    for name in ("qe_affine_relu_quantize_pack", "qe_affine_relu_quantize_pack_path"):
        assert name in capi.PROTOTYPES and hasattr(capi.lib(), name)
    assert capi.PREACT_KERNELS == ("plain", "fast")
    assert not any("affine_relu" in n and n.endswith(("workspace_bytes", "prepared_bytes")) for n in capi.PROTOTYPES)


def test_the_path_query_reaches_both_instances_in_every_epilogue_form():
    seen = set()
    for k, row in enumerate(pi.ROWS):
        assert pi.expected_instance(k, 2) == row[0], pi.row_id(k)
        for n_out in (0, 1, 2):
            for sum_ptr, act_ptr in ((256, 0), (0, 256), (256, 256)) + (((0, 0),) if n_out else ()):
                got = pi.path(k, n_out, sum_ptr, act_ptr)
                assert got >= 0 and capi.PREACT_KERNELS[got] == pi.expected_instance(k, n_out), (pi.row_id(k), n_out, sum_ptr, act_ptr)
                seen.add((capi.PREACT_KERNELS[got], n_out, bool(sum_ptr), bool(act_ptr)))
    forms = {(n, s, a) for n in (0, 1, 2) for s in (False, True) for a in (False, True) if n or s or a}
    assert seen == {(i, *f) for i in capi.PREACT_KERNELS for f in forms}


def test_the_instance_does_not_depend_on_an_alignment():
    for k in range(len(pi.ROWS)):
        for n_out in (0, 1, 2):
            want = pi.path(k, n_out, 256, 256)
            for sum_ptr, act_ptr in ((260, 268), (4, 257 * 4), (256 + 12, 256 + 8)):
                assert pi.path(k, n_out, sum_ptr, act_ptr) == want, (pi.row_id(k), n_out)


def test_refused_requests_have_no_instance():
    rq8, rq9 = pi.fake_rq("u8", 3), capi.requant(pi._Fake(1), pi._Fake(1), 0, 255, 9, 0)
    assert capi.affine_relu_quantize_pack_path(2, 3, 64, [rq8]) == 1
    assert capi.affine_relu_quantize_pack_path(2, 3, 64, [], sum_out=0, act_out=0) == -1            # no output requested
    assert capi.affine_relu_quantize_pack_path(2, 3, 64, [rq9]) == -1                               # n_bits
    assert capi.affine_relu_quantize_pack_path(2, 3, 64, [rq8, rq8, rq8]) == -1                     # n_out
    assert capi.affine_relu_quantize_pack_path(2, 3, 0, [rq8]) == -1 and capi.affine_relu_quantize_pack_path(0, 3, 64, [rq8]) == -1
    assert capi.affine_relu_quantize_pack_path(2, 4, 64, [pi.fake_rq("s8c", 3)]) == -1              # n_param neither 1 nor C
    assert capi.affine_relu_quantize_pack_path(2, 3, 64, [capi.QeRequant(None, 256, 1, 0.0, 255.0, 8, 0)]) == -1


# ---- the reference's own chain ---------------------------------------------------------------------------------------------
def _boundary(g14, key):
    g = lambda f: g14.get(key, f)
    alpha, shift = preact_ref.bn_affine(g("bn_weight"), g("bn_bias"), g("bn_mean"), g("bn_var"), float(g("bn_eps")))
    n = int(g("n_out"))
    rqs = []
    for i in range(n):
        qmin, qmax = float(g("q%d_qmin" % i)), float(g("q%d_qmax" % i))
        bits = max(1, int(round(qmax - qmin)).bit_length())
        rqs.append((g("q%d_scale" % i).reshape(-1), g("q%d_zero" % i).reshape(-1), qmin, qmax, bits, int(qmin < 0)))
    N, C, H, W = g("x").shape
    x, identity = g("x").reshape(N, C, H * W), g("identity").reshape(N, C, H * W)
    return x, identity, alpha, shift, rqs, [g("q%d_q" % i).reshape(N, C, H * W) for i in range(n)]


def test_preact_ref_reproduces_g14_boundaries(g14):
    keys = [k for k in g14.index if k.startswith("b_")]
    assert sorted(keys) == ["b_pc", "b_two", "b_u8"]
    for key in keys:
        x, identity, alpha, shift, rqs, want = _boundary(g14, key)
        assert len(rqs) == (2 if key == "b_two" else 1) and (rqs[0][0].size > 1) == (key == "b_pc")
        ref = preact_ref.forward(x, identity, alpha, shift, rqs)
        assert not ref["flag"], key
        for i, (q, w) in enumerate(zip(ref["q"], want)):
            differ = q != w
            excused = preact_ref.tie_excused(x, identity, alpha, shift, rqs[i][0], rqs[i][1])
            print("%s consumer %d: %d of %d codes differ, %d elements near a tie" % (key, i, differ.sum(), q.size, excused.sum()))
            assert not (differ & ~excused).any(), key
            # the fixture is chosen so that nothing needs the excuse: the generator checks it, and so does this
            assert not excused.any(), key
            assert not differ.any(), key
            assert len(np.unique(w)) > (1 << rqs[i][4]) // 8, key          # the codes use a real part of the range


def test_bn_affine_is_atens_eval_mode_batch_norm(g14):
    import torch
    x, identity, alpha, shift, rqs, _ = _boundary(g14, "b_pc")
    g = lambda f: torch.from_numpy(np.asarray(g14.get("b_pc", f)))
    s = torch.from_numpy(x + identity).reshape(g("x").shape)
    want = torch.nn.functional.batch_norm(s, g("bn_mean"), g("bn_var"), g("bn_weight"), g("bn_bias"), False, 0.0, float(g("bn_eps")))
    got = preact_ref.activated(x, identity, alpha, shift)[1].reshape(want.shape)
    err = np.abs(got.astype(np.float64) - torch.relu(want).numpy().astype(np.float64))
    # two fp32 evaluations of the same affine: ATen may fuse it, the contract does not
    bound = 4 * 2.0 ** -24 * (np.abs(s.numpy()) * np.abs(alpha).reshape(1, -1, 1, 1) + np.abs(shift).reshape(1, -1, 1, 1))
    assert (err <= bound).all()


# ---- the contract against its two nearly-right evaluations -------------------------------------------------------------------
def test_the_tie_dense_input_tells_the_contract_from_an_fma_and_from_float64():
    t = pi.tie_dense()
    got = {m: preact_ref.forward(t["x"], None, t["alpha"], t["shift"], [t["rq"]], mode=m) for m in ("contract", "fma", "f64")}
    n = t["x"].size
    assert not got["contract"]["flag"]
    d_fma = int((got["contract"]["q"][0] != got["fma"]["q"][0]).sum())
    d_f64 = int((got["contract"]["q"][0] != got["f64"]["q"][0].astype(np.float32)).sum())
    print("tie-dense: %d elements, %d codes differ from the FMA form, %d from float64" % (n, d_fma, d_f64))
    assert d_fma >= n // 20 and d_f64 >= n // 20
    # and the affine itself: s * alpha + shift rounded twice is not the FMA's bits
    assert (got["contract"]["a"] != got["fma"]["a"]).sum() >= n // 20


def test_the_grid_cap_case_runs_the_loop_twice():
    N, C, P = pi.beyond_the_grid_cap()
    groups = -(-N * C * P // pi.PLAIN_VEC)
    assert pi.GRID_CAP * pi.THREADS < groups <= 2 * pi.GRID_CAP * pi.THREADS
    assert capi.affine_relu_quantize_pack_path(N, C, P, [pi.fake_rq("u8", C)]) == 0
