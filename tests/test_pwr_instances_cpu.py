"""CPU: the resident-tile instance table (tests/pwr_instances.py) names the instance the launcher dispatches each row to,
and together its rows reach every instance the launchers can select: 24 plain / re-quantising conv_pwr_kernel, 12
residual, 6 plain / re-quantising conv_pwr7_kernel and 2 residual."""
import os
import re

import pwr_instances as pi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rows_name_their_dispatched_instance():
    for shape, base, note, _ in pi.ROWS:
        assert pi.instance(shape) == base, "%s (%s): the launcher dispatches it to %s" % (shape, note, pi.instance(shape))


def test_rows_cover_every_instance():
    every = pi.dispatchable()
    kinds = lambda k, res: sum(1 for i in every if i[0] == k and i[-1] == res)
    assert (kinds(pi.PWR, False), kinds(pi.PWR, True), kinds(pi.PWR7, False), kinds(pi.PWR7, True)) == (24, 12, 6, 2)
    missing = every - pi.covered()
    assert not missing, "no row reaches %s" % sorted(pi.kernel_name(i) for i in missing)
    assert pi.covered() <= every


def test_rows_vary_the_branch_conditions():
    shapes = [r[0] for r in pi.ROWS]
    assert any(N == 1 for N, *_ in shapes) and any(N % 2 == 1 and N > 1 for N, *_ in shapes)
    assert {448, 1120, 4480} <= {H * W for N, IC, H, W, OC, K, s, p in shapes if s == 1}
    assert any(r[3] and "QE_PWR_GROUPS" in r[3] for r in pi.ROWS)


def test_kernel_names_match_the_launcher_templates():
    """The names the trace check looks for are spelled as the launcher instantiates them."""
    src = open(os.path.join(REPO, "quantize_amd", "csrc", "qe_conv_pwr.hip")).read()
    assert re.search(r"conv_pwr_kernel<7, WV, KSV, TWV, S2V, RQV>", src)
    assert re.search(r"conv_pwr_kernel<7, WV, KSV, TWV, false, RQV, true>", src)
    assert re.search(r"conv_pwr7_kernel<KSV, GIV, RQV, RESV>", src)
    assert pi.kernel_name((pi.PWR, 4, 2, 224, True, True, False)) == "conv_pwr_kernel<7, 4, 2, 224, true, true, false>"
    assert pi.kernel_name((pi.PWR7, 16, 2, False, True)) == "conv_pwr7_kernel<16, 2, false, true>"
