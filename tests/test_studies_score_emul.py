"""CPU checks of the strip scoring kernel's ARITHMETIC (csrc/gp_studies_score.h: sa_score_strip, the body of
scaml_target_score_batched_kernel) through a host build of the same source (tests/host_emul/studies_score_emul.cpp), next to a host
build of ``sa_query`` (csrc/gp_studies_acqf.h) in the same library.  Both are fed the same numbers (tests/_studies_score_problem.py):
the strip side in the value layout, the ``sa_query`` side in column 0 of its 16-column layout with NaN in columns 1 .. 15.  ``value``,
``mu`` and ``var`` must be equal BIT FOR BIT, and both agree with a torch-fp64 restatement within the tolerance
tests/test_studies_acqf_emul.py holds ``sa_query`` to (value, mu rtol 1e-9; var rtol 1e-9, atol 1e-12).

One batch of studies with n = 1, 15, 16, 17, 33 (n_max = 33) and a study whose info is 1; T = 3 and 9 (across the eight-task chunk);
D = 2 and 6; both kernel families; UCB and EI.  What is planted is listed in tests/_studies_score_problem.py.  The parallel execution
is what tests/test_studies_score_gpu.py covers."""
import ctypes

import numpy as np
import pytest
import torch

torch.set_num_threads(1)

from tests import _studies_score_problem as SP
from tests._host_emul import BP, DP, IP, build, ptr as _p

ARGTYPES = [DP, DP, DP, IP, DP, DP, BP, DP, DP, DP, DP, DP, IP, DP, DP, IP, DP] + [ctypes.c_int] * 7 + [DP] * 3


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    lib = build(tmp_path_factory, "studies_score_emul")
    for fn in (lib.emul_studies_score, lib.emul_studies_acqf_value):
        fn.restype, fn.argtypes = ctypes.c_int, ARGTYPES
    return lib


def _run(fn, prob, acqf, layout):
    a = prob.arrays(acqf, layout)
    Mq = prob.Mq
    out = dict(value=np.full(Mq, 7.0), mu=np.full(Mq, 7.0), var=np.full(Mq, 7.0))
    rc = fn(*[_p(a[k]) for k in SP.ORDER], Mq, prob.G, prob.n_max, prob.T, prob.D, prob.kind, acqf, _p(out["value"]), _p(out["mu"]), _p(out["var"]))
    assert rc == 0
    return out


@pytest.mark.parametrize("T", [3, 9])
@pytest.mark.parametrize("D", [2, 6])
@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("acqf", [0, 1])
def test_strip_kernel_equals_sa_query_bit_for_bit_and_matches_torch(emul, T, D, kind, acqf):
    prob = SP.Problem(T, D, kind, seed=300 + 10 * T + D + kind, strips=(1, 1, 3, 1, 1, 1))
    strip = _run(emul.emul_studies_score, prob, acqf, "value")
    query = _run(emul.emul_studies_acqf_value, prob, acqf, "grad")
    for k in ("value", "mu", "var"):
        assert strip[k].tobytes() == query[k].tobytes(), k          # bit for bit, NaN included
    for q in range(prob.Mq):
        s_ = prob.study_of(q)
        got = [strip[k][q] for k in ("value", "mu", "var")]
        if s_ < 0:                                                 # the padding strip
            assert got == [0.0, 0.0, 0.0], (q, got)
        elif s_ == SP.FAILED or q == prob.nan_q:                   # info = 1; the candidate with a NaN coordinate
            assert np.isnan(got).all(), (q, got)
        else:
            val, mu, var = prob.reference(acqf, q)
            np.testing.assert_allclose(got[0], val, rtol=1e-9, err_msg=f"value q={q}")
            np.testing.assert_allclose(got[1], mu, rtol=1e-9, err_msg=f"mu q={q}")
            np.testing.assert_allclose(got[2], var, rtol=1e-9, atol=1e-12, err_msg=f"var q={q}")
    # the NaN coordinate spoils its own candidate only: its strip's other 15 candidates are finite
    rest = [q for q in range(16 * (prob.nan_q // 16), 16 * (prob.nan_q // 16) + 16) if q != prob.nan_q]
    assert np.isfinite(strip["value"][rest]).all()


def test_lds_footprint_holds_the_carve_and_fits(emul):
    emul.emul_studies_score_lds_doubles.restype, emul.emul_studies_score_lds_doubles.argtypes = ctypes.c_longlong, [ctypes.c_int]
    for n in range(1, 97):
        nb = (n + 15) // 16
        assert emul.emul_studies_score_lds_doubles(n) == n * 16 + 32 + 2 * 16 * nb * 16 + 16 * nb + 256 * nb + n * (n | 1) + 32
    assert emul.emul_studies_score_lds_doubles(96) * 8 <= 160 * 1024
