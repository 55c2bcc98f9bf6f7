"""CPU: every edge of the launcher's dispatch rules (csrc/gp_dispatch.h, through tests/_dispatch.py) pinned with literal expected values,
at 256 CUs (the MI355X) and again at 64 -- nothing in the rules may have a CU count baked in except the named constant of the
inverse-factor split.  csrc/scaml_host.cpp launches from these very functions, so a rule that moves fails here and nowhere silently:
the helpers that name the instance a case exercises (tests/_fit_bounds.py, tests/_failpath_cases.py, tests/_target_fit_bounds.py) ask
the same plans."""
from types import SimpleNamespace

import pytest

from tests import _dispatch as DP

KIB = 1024
FIT = {0: (0, 2, 1, 128), 1: (1, 4, 3, 256), 2: (2, 8, 3, 256), 3: (3, 16, 7, 512), 4: (4, 8, 7, 512)}      # variant -> (variant, nb, wu, block)


def test_constants():
    assert DP.LDS_LIMIT == 160 * KIB
    assert DP.LINV_TARGET_WORKGROUPS == 256


def test_python_studies_limits_are_the_headers():
    """scamlgp_amd/studies.py restates csrc/gp_studies_acqf.h's limits for the Python layer (the stack's N: tests/test_studies_acqf_gpu.py)."""
    from scamlgp_amd import studies

    assert (studies.MAX_N, studies.MAX_D, studies.MAX_FANTASIES) == (DP.STUDIES_MAX_N, DP.STUDIES_MAX_D, DP.STUDIES_MAX_FANTASIES)


def _model(n=8, D=2, N=32, num_fantasies=None, device="cuda"):
    """What ``studies.takes`` reads of a ScaMLGP."""
    return SimpleNamespace(n=n, num_fantasies=num_fantasies, device=SimpleNamespace(type=device), _stack=SimpleNamespace(D=D, N=N))


def test_studies_predicate_at_its_edges():
    from scamlgp_amd.studies import takes

    # the model as it stands: 1 <= n <= 96 (its stack's N does not bound n), D <= 15, N <= 512, on the GPU, at most 64 fantasies
    assert [takes(_model(n=n)) for n in (0, 1, 96, 97)] == [False, True, True, False]
    assert [takes(_model(D=D)) for D in (15, 16)] == [True, False]
    assert [takes(_model(N=N)) for N in (512, 513)] == [True, False]
    assert takes(_model(n=40, N=32)) and not takes(_model(device="cpu"))
    assert [takes(_model(num_fantasies=F)) for F in (None, 1, 64, 65)] == [True, True, True, False]
    # an ordinary model still to be conditioned on p points with F fantasies: n + p <= 96 and <= N, 1 <= F <= 64
    assert [takes(_model(n=n, N=128), p, 4) for n, p in ((0, 1), (1, 1), (95, 1), (96, 1), (90, 6), (90, 7))] == [False, True, True, False, True, False]
    assert [takes(_model(n=30, N=32), p, 4) for p in (2, 3)] == [True, False]
    assert [takes(_model(n=8), 1, F) for F in (0, 1, 64, 65)] == [False, True, True, False]
    assert [takes(_model(n=8, D=D), 1, 4) for D in (15, 16)] == [True, False]
    assert not takes(_model(n=8, num_fantasies=4), 1, 4) and not takes(_model(n=8, device="cpu"), 1, 4)   # (a fantasy model is not conditioned further)


# ---- fused fit / POTRF ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cus", [256, 64])
def test_fit_size_classes(cus):
    for N, cls, variant in [(1, 0, 0), (32, 0, 0), (33, 1, 1), (64, 1, 1), (65, 2, 4), (128, 2, 4), (129, 3, 3), (256, 3, 3)]:
        assert DP.fit_class(N) == cls, N
        for T in (1, cus):
            assert DP.fit_plan(T, N, 1, cus)[:4] == FIT[variant], (T, N)
    assert [DP.fit_plan(1, N, 1, cus).lds_doubles for N in (32, 64, 128, 256)] == [4018, 6336, 11068, 20404]


@pytest.mark.parametrize("cus", [256, 64])
def test_fit_narrow_instance_past_the_cu_count(cus):
    """64 < N <= 128 alone: the wide (8, 7) up to #CUs tasks, the narrow (8, 3) from #CUs + 1."""
    for N in (65, 128):
        assert DP.fit_plan(cus, N, 8, cus) == FIT[4] + (11074,)
        assert DP.fit_plan(cus + 1, N, 8, cus) == FIT[2] + (10946,)
    for N, variant in [(64, 1), (129, 3)]:
        assert DP.fit_plan(cus + 1, N, 8, cus)[:4] == FIT[variant]
    assert DP.narrow_fit_tasks(cus) == cus + 1


def test_fit_narrow_instance_at_256_cus():
    assert DP.fit_plan(256, 128, 8, 256)[1:3] == (8, 7) and DP.fit_plan(257, 128, 8, 256)[1:3] == (8, 3)


@pytest.mark.parametrize("cus", [256, 64])
def test_fit_largest_d_per_class(cus):
    """scaml_fit_max_d per class (sized for the largest instance's row lists, D in steps of 4) and the LDS request there; the plan's
    own footprint passes 160 KiB at `over`, one above for the N <= 256 class (TOOLARGE from the launcher)."""
    for N, dmax, lds, over in [(32, 592, 19936, 609), (64, 296, 19910, 305), (128, 144, 19882, 149), (256, 44, 20446, 45)]:
        assert DP.fit_class_max_d(N) == dmax and DP.fit_class_max_d(N // 2 + 1) == dmax
        p = DP.fit_plan(1, N, dmax, cus)
        assert p.lds_doubles == lds and lds * 8 <= DP.LDS_LIMIT
        assert DP.fit_plan(1, N, over - 1, cus).lds_doubles * 8 <= DP.LDS_LIMIT < DP.fit_plan(1, N, over, cus).lds_doubles * 8, N
    assert DP.fit_plan(cus + 1, 128, 144, cus).lds_doubles == 19754      # the narrow instance: fewer row lists
    assert DP.fit_plan(1, 256, 45, cus).lds_doubles == 20928


# ---- blocked fit ---------------------------------------------------------------------------------------------------
# (T, N) -> parts, path by shape; at 256 CUs, and the same edges at 64
BLOCKED = {
    256: [((2, 512), 8, 2), ((85, 512), 3, 2), ((86, 512), 2, 1), ((128, 512), 2, 1), ((128, 320), 2, 2), ((128, 336), 2, 1), ((129, 320), 1, 1),
          ((1, 272), 8, 2)],
    64: [((2, 512), 8, 2), ((21, 512), 3, 2), ((22, 512), 2, 1), ((32, 512), 2, 1), ((32, 320), 2, 2), ((32, 336), 2, 1), ((33, 320), 1, 1),
         ((1, 272), 8, 2), ((65, 320), 0, 1)],
}


@pytest.mark.parametrize("cus", [256, 64])
def test_blocked_path_by_shape_and_by_mode(cus):
    for (T, N), parts, path in BLOCKED[cus]:
        for D in (16, 17):
            for mode in (0, 1, 2):
                p = DP.blocked_plan(T, N, D, cus, mode)
                want = 1 if D == 17 or mode == 1 else (path if mode == 0 else (2 if parts >= 1 else 1))
                assert (p.parts, p.path) == (parts, want), (T, N, D, mode)
                assert p.t8 == (T + 7) // 8 * 8


def test_blocked_parts_are_capped_by_block_columns():
    assert DP.blocked_plan(1, 272, 3, 256).parts == 8 and DP.blocked_plan(1, 272, 3, 64).parts == 8      # 9 block columns, at most 8
    assert DP.blocked_plan(1, 272, 3, 7).parts == 7 and DP.blocked_plan(1, 272, 3, 2).path == 2          # two workgroups, N <= 320


@pytest.mark.parametrize("cus", [256, 64])
def test_blocked_workspace_and_geometry(cus):
    p = DP.blocked_plan(2, 512, 8, cus)
    assert p == (2, 8, 8, 88896, 352, 9568, 4, 1, 4, 141128, 42568)
    assert p.flag_bytes == 2 * 44 * 4 and p.need == 352 + 2 * 512 * 8 + 2 * 64 * 8
    assert DP.blocked_plan(2, 512, 8, cus, 0, p.need).path == 2
    assert DP.blocked_plan(2, 512, 8, cus, 0, p.need - 1).path == 1       # a workspace one byte short: the sequence of launches
    assert DP.blocked_plan(2, 512, 8, cus, 2, p.need - 1).path == 1
    assert DP.blocked_plan(3, 272, 9, cus).flag_bytes == 528               # 3 * 176 = 528, a multiple of 16; T = 1: 176
    assert DP.blocked_plan(1, 272, 9, cus)[4:6] == (176, 176 + 272 * 8 + 512)
    # the sequence: tiles of 64 rows of the second block, the solve's SMALLD, the rounds of the jitter ladder
    assert [DP.blocked_plan(1, N, 8, cus).nt for N in (272, 320, 336, 384, 400, 512)] == [1, 1, 2, 2, 3, 4]
    assert [DP.blocked_plan(1, 512, D, cus).solve_small_d for D in (8, 9)] == [1, 0]
    assert DP.blocked_plan(1, 512, 8, cus, no_retry=True).rounds == 1 and DP.blocked_plan(1, 512, 8, cus).rounds == 4
    assert DP.blocked_plan(1, 512, 9, cus)[9:] == (17642 * 8, 5322 * 8) == (141136, 42576) and DP.blocked_plan(1, 512, 17, cus)[9:] == (161680, 50832)


def test_blocked_one_launch_asks_for_more_than_half_a_cus_lds():
    """The request never falls below 82 KiB (one workgroup per CU); above it, the kernel's own footprint."""
    assert [DP.blocked_plan(1, N, D, 256).lds_coop for (N, D) in ((272, 1), (272, 8), (512, 1))] == [82 * KIB] * 3
    assert [DP.blocked_plan(1, N, D, 256).lds_coop for (N, D) in ((272, 16), (512, 8), (512, 16))] == [89024, 88896, 121664]


# ---- MLL gradient --------------------------------------------------------------------------------------------------
FUSED_LDS = {0: 2306, 1: 4460, 2: 8768, 3: 17384}      # doubles, per size class
TWO_LDS = {8: 2304, 9: 2816}                            # doubles, per D


def _single(T, sc, dma, split=1):
    nbt = 2 << sc
    return (1, sc, nbt, dma, split, T, split, nbt * 32 // split, FUSED_LDS[sc])


@pytest.mark.parametrize("cus", [256, 64])
def test_grad_size_classes_and_staging(cus):
    T = 2 * cus      # (past every small-stack and split rule)
    for N, sc, dma in [(32, 0, 1), (33, 1, 0), (64, 1, 1), (65, 2, 0), (128, 2, 1), (129, 3, 0), (256, 3, 1)]:
        assert DP.grad_plan(T, N, 8, cus) == _single(T, sc, dma), N
        assert DP.grad_plan(T, N, 8, cus, ragged=True) == _single(T, sc, 0), N
        assert DP.grad_plan(T, N, 8, cus, aligned16=False) == _single(T, sc, 0), N
        assert not DP.grad_plan(T, N, 9, cus).single and not DP.grad_plan(T, N, 8, cus, mode=1).single
    for mode in (0, 1, 2):
        assert not DP.grad_plan(T, 257, 8, cus, mode).single


@pytest.mark.parametrize("cus", [256, 64])
def test_grad_small_stack_takes_two_launches(cus):
    """N > 64 and T <= 64 (a task count, not a CU count): two launches by shape, the single launch only when forced or with
    SCAML_GRAD_NO_SPLIT."""
    for N, sc, dma in [(64, 1, 1), (65, 2, 0)]:
        for T in (64, 65):
            small = N > 64 and T <= 64
            assert DP.grad_plan(T, N, 8, cus).single == (not small), (T, N)
            assert DP.grad_plan(T, N, 8, cus, mode=2) == _single(T, sc, dma)
            assert DP.grad_plan(T, N, 8, cus, no_split=True) == _single(T, sc, dma)
            assert not DP.grad_plan(T, N, 8, cus, mode=1, no_split=True).single
    assert DP.grad_plan(64, 128, 8, cus) == (0, 0, 0, 0, 0, 64 * 3, 1, 256, 2304)      # nb = 8: 10 super-tiles, 3 groups of four waves
    assert DP.grad_plan(64, 128, 9, cus, mode=2) == (0, 0, 0, 0, 0, 64 * 3, 1, 256, 2816)


def test_grad_split_at_256_cus():
    """The N <= 256 class staged by LDS-DMA, while two workgroups per task fit the CUs: T <= 128."""
    assert DP.grad_plan(128, 256, 8, 256) == _single(128, 3, 1, split=2) == (1, 3, 16, 1, 2, 128, 2, 256, 17384)
    assert DP.grad_plan(129, 256, 8, 256) == _single(129, 3, 1) == (1, 3, 16, 1, 1, 129, 1, 512, 17384)
    assert DP.grad_plan(65, 256, 8, 256).split == 2
    for kw in (dict(ragged=True), dict(aligned16=False), dict(no_split=True)):
        assert DP.grad_plan(65, 256, 8, 256, **kw).split == 1, kw
    assert DP.grad_plan(65, 128, 8, 256).split == 1 and DP.grad_plan(65, 240, 8, 256).split == 2
    assert DP.grad_plan(2, 256, 8, 256, mode=2).split == 2 and not DP.grad_plan(2, 256, 8, 256).single


def test_grad_split_at_64_cus():
    """2 T <= 64 lies inside the small stacks: by shape those take two launches, the split shows only when the single launch is forced."""
    assert not DP.grad_plan(32, 256, 8, 64).single
    assert DP.grad_plan(32, 256, 8, 64, mode=2) == _single(32, 3, 1, split=2)
    assert DP.grad_plan(33, 256, 8, 64, mode=2) == _single(33, 3, 1)
    assert DP.grad_plan(65, 256, 8, 64) == _single(65, 3, 1) and DP.grad_plan(128, 256, 8, 64).split == 1


@pytest.mark.parametrize("cus", [256, 64])
def test_grad_two_launch_grid(cus):
    """ceil(T / 8) * 8 tasks times groups of four 2 x 2 super-tiles; nb odd and even."""
    for N, nb, groups in [(16, 1, 1), (32, 2, 1), (48, 3, 1), (64, 4, 1), (272, 17, 12), (288, 18, 12), (304, 19, 14), (496, 31, 34), (512, 32, 34)]:
        assert (N + 15) // 16 == nb
        for T, t8 in [(3, 8), (8, 8), (9, 16)]:
            for D in (8, 9):
                assert DP.grad_plan(T, N, D, cus, mode=1) == (0, 0, 0, 0, 0, t8 * groups, 1, 256, TWO_LDS[D]), (T, N, D)


# ---- target-GP fit -------------------------------------------------------------------------------------------------
def test_target_fit_path():
    assert DP.target_fit_plan(112, 4, 6) == (1, 16816) and DP.target_fit_plan(113, 4, 6) == (0, 14592)
    assert DP.target_fit_plan(112, 4, 6, mode=1) == (0, 14353)                     # the debug mode: column by column
    assert DP.target_fit_plan(112, 1000, 16) == (1, 19958)
    assert DP.target_fit_plan(112, 2000, 16) == (0, 19495)                         # n <= 112 whose matrix-core footprint passes 160 KiB
    assert 21958 * 8 > DP.LDS_LIMIT >= 19495 * 8
    assert DP.target_fit_plan(96, 3000, 16) == (1, 19798) and DP.target_fit_plan(96, 4000, 16) == (0, 19783)


def test_target_fit_batched_path():
    """A batch straddling 112: each problem is factorised by its own n, the LDS is the largest footprint any n <= n_max asks for."""
    assert DP.target_fit_plan(113, 4, 6, batched=True) == (1, 16816)               # n = 112 on the matrix cores is the largest
    assert DP.target_fit_plan(128, 4, 6, batched=True) == (1, DP.target_fit_plan(128, 4, 6).lds_doubles) == (1, 18417)
    assert DP.target_fit_plan(112, 4, 6, batched=True) == (1, 16816)
    assert DP.target_fit_plan(113, 4, 6, mode=1, batched=True) == (0, 14592)


# ---- posteriors, strip solves, inverse factor ------------------------------------------------------------------------
def test_posterior_waves_and_staging():
    """The first D of each configuration, (waves, X staged): 4 -> 2 -> 1 waves, staged before unstaged at each count."""
    want = {16: [(1, 4, 1), (240, 4, 0), (299, 2, 1), (406, 2, 0), (603, 1, 1), (611, 1, 0), (1185, 0, 1)],
            256: [(1, 4, 1), (12, 4, 0), (59, 2, 0), (363, 1, 0), (945, 0, 1)],
            512: [(1, 2, 1), (7, 2, 0), (107, 1, 0), (689, 0, 1)]}
    for N, edges in want.items():
        for (D, waves, xl), nxt in zip(edges, edges[1:] + [None]):
            assert DP.posterior_plan(N, D) == (waves, xl), (N, D)
            if nxt:
                assert DP.posterior_plan(N, nxt[0] - 1) == (waves, xl), (N, nxt[0] - 1)
    assert DP.posterior_plan(257, 1) == DP.posterior_plan(272, 1) == (4, 1) and DP.posterior_plan(304, 1).waves == 4 and DP.posterior_plan(320, 1).waves == 2


def test_strip_solve_waves():
    assert [DP.strip_solve_waves(np_) for np_ in (16, 320, 336, 512, 640, 656)] == [4, 4, 2, 2, 2, 1]


def test_linv_groups():
    """Doubling while every wave keeps a strip and T * groups stays within 256 workgroup slots -- the named constant, whatever the device."""
    cases = [(1, 4, 1), (8, 4, 2), (16, 4, 4), (32, 2, 16), (32, 4, 8), (21, 2, 8)]      # (nb, waves) -> groups at T = 1
    want = {1: [1, 2, 4, 16, 8, 8], 32: [1, 2, 4, 8, 8, 8], 64: [1, 2, 4, 4, 4, 4], 128: [1, 2, 2, 2, 2, 2], 129: [1, 1, 1, 1, 1, 1]}
    for T, groups in want.items():
        assert [DP.linv_groups(T, nb, waves) for nb, waves, _ in cases] == groups, T
    assert [g for _, _, g in cases] == want[1]
