"""Host-side: the rule that sends a fused fit to the full-tile instance gp_fit_fused_kernel<16, 7, kind, true>
(fit_full_instance, csrc/gp_dispatch.h), through the header compiled as host code (tests/_fit_full.py).  Inside the kernel every
clause of the contract is a compile-time fact, so a call that breaks one and is still sent there would read or write out of
bounds: each clause is switched off in turn, next to the call that satisfies all of them."""
import pytest

from tests import _fit_full as F
from tests._dispatch import fit_plan

CUS = 256
ALIGNED, ODD8 = 0x7F0000001000, 0x7F0000001008


def test_the_flagship_call_takes_the_full_instance():
    assert F.fit_full_instance(16, 7, 256)
    assert F.fit_full_instance(16, 7, 256, l_addr=ALIGNED)
    for T in (1, 3, 256, 4096):
        for D in (1, 8, 20, 21, 44):
            assert F.fit_full_of_call(T, 256, D, CUS, l_addr=ALIGNED), (T, D)


@pytest.mark.parametrize("clause,kw", [
    ("n_points given", dict(ragged=True)),
    ("a given matrix (POTRF mode)", dict(from_matrix=True)),
    ("a diagonal block of a blocked fit", dict(blocked=True)),
    ("L on an 8-byte boundary only", dict(l_addr=ODD8)),
    ("L one byte off", dict(l_addr=ALIGNED + 1)),
    ("the switch set to never", dict(mode=1)),
])
def test_each_clause_false_in_turn(clause, kw):
    assert F.fit_full_instance(16, 7, 256, **{"l_addr": ALIGNED, **kw}) is False, clause
    assert F.fit_full_of_call(3, 256, 8, CUS, **{"l_addr": ALIGNED, **kw}) is False, clause


@pytest.mark.parametrize("N", [1, 16, 240, 241, 255])
def test_padded_rows_keep_the_generic_instance(N):
    assert F.fit_full_instance(16, 7, N, l_addr=ALIGNED) is False
    assert F.fit_full_of_call(3, N, 8, CUS, l_addr=ALIGNED) is False


@pytest.mark.parametrize("nb,wu", [(2, 1), (4, 3), (8, 3), (8, 7)])
def test_the_other_size_classes_have_no_full_instance(nb, wu):
    """... at their own full size N = 16 nb, and whatever N says."""
    assert F.fit_full_instance(nb, wu, 16 * nb, l_addr=ALIGNED) is False
    assert F.fit_full_instance(nb, wu, 256, l_addr=ALIGNED) is False
    for T in (1, 3, CUS + 1):
        p = fit_plan(T, 16 * nb, 8, CUS)
        assert F.fit_full_of_call(T, 16 * nb, 8, CUS, l_addr=ALIGNED) is False, p
    assert F.fit_full_instance(16, 3, 256, l_addr=ALIGNED) is False      # (no such instance: both template arguments are tested)


def test_alignment_only_counts_when_l_is_stored():
    """store_L off: nothing is written through L, whatever the pointer is."""
    assert F.fit_full_instance(16, 7, 256, stores_l=False, l_addr=ODD8)
    assert F.fit_full_instance(16, 7, 256, stores_l=False, l_addr=0)
    assert F.fit_full_instance(16, 7, 256, stores_l=True, l_addr=ODD8) is False


def test_switch_values():
    """Only mode 0 admits the instance (1 is `never`: what the launcher passes when SCAML_FIT_NO_FULL is set)."""
    assert F.fit_full_instance(16, 7, 256, mode=0) and not F.fit_full_instance(16, 7, 256, mode=1)
    assert not F.fit_full_instance(16, 7, 256, mode=2) and not F.fit_full_instance(16, 7, 256, mode=-1)
