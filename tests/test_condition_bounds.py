"""CPU: the host build of the studies' batched fantasy set-up (csrc/gp_studies_condition.h through
tests/host_emul/studies_condition_emul.cpp) held, element by element, to the a-priori bounds of tests/_condition_bounds.py against a
long-double reference fed with the SAME inputs -- (7m) the synthetic source pass of tests/test_studies_condition_emul.py, (7n) the same
L', resid, mean_p and eps.  The groups are that file's; the largest error / bound ratio per output is printed (``pytest -s``)."""
import numpy as np
import pytest

from tests import _condition_bounds as C
from tests import _target_bounds as TB
from tests.test_studies_condition_emul import GROUPS, INFO_GROUP, NAN_GROUP, NOFANT_GROUP, Problem, factor, load, run_block, run_fantasy


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    return load(tmp_path_factory)


@pytest.mark.parametrize("kind", [0, 1], ids=["rbf", "matern"])
@pytest.mark.parametrize("D", [1, 6, 15])
def test_host_build_within_the_bounds(emul, D, kind):
    prob = Problem(D, kind, seed=300 + 10 * D + kind)
    a = prob.block_arrays()
    blk = run_block(emul, prob, a)
    L = factor(prob, blk)
    eps = prob.eps_array()
    out = run_fantasy(emul, prob, a, blk, L, eps)
    for s_, (no, p, F) in enumerate(GROUPS):
        n, c0 = no + p, 16 * int(prob.base[s_])
        label = f"D = {D} {C.FAMILY[kind]} group {s_} (n_obs, p, F) = {(no, p, F)}"
        rb = C.block_reference(a["mu"][:, c0:c0 + n], a["cov"][:, :n, c0:c0 + n], np.nan_to_num(a["w"][s_]), a["active"][s_], a["Xt"][s_, :n],
                               a["theta"][s_], a["y"][s_], no, a["m_all"][s_], a["s_all"][s_], kind)
        got_b = dict(Knn=blk["Knn"][s_, :n, :n], resid=blk["resid"][s_, :n], mean_p=blk["mean_p"][s_, :n])
        if s_ in (INFO_GROUP, NOFANT_GROUP):   # (7n) refuses them: (7m) alone
            C.check_study(label, kind, got_b, None, rb, None, no)
            continue
        rf = C.fantasy_reference(L[s_, :n, :n], blk["resid"][s_, :n], blk["mean_p"][s_, :n], eps[s_, :p, :max(F, 1)], no, a["m_all"][s_], a["s_all"][s_])
        got_f = dict(alpha_f=out["alpha_f"][s_, :n, :F], y_fant=out["y_fant"][s_, :p, :F], mu_p=out["mu_p"][s_, :p])
        C.check_study(label, kind, got_b, got_f, rb, rf, no)
    assert NAN_GROUP < len(GROUPS)   # (its coordinates are finite here: the NaN rule is tests/test_studies_condition_emul.py's)
    for line in TB.report("condition_block") + TB.report("fantasy_condition"):
        print(line)
