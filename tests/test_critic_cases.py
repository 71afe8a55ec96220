"""The critic sweep's case table (tests/critic_cases.py) without a GPU: it reaches every cell of the critic step's
dispatch map, the coverage check sees a missing cell, and every case's inputs stay where the fp32-against-fp64
comparison of tests/test_gpu_critic_sweep.py is valid (no saturated sigmoid, no head row at a relu kink)."""

import numpy as np
import pytest

import critic_cases as cc
import gan_mpc_oracle as orc


def test_case_table_covers_the_dispatch_map():
    assert cc.missing_cells(cc.CASES) == []


@pytest.mark.parametrize("cell", cc.required_cells(), ids=str)
def test_coverage_check_sees_a_missing_cell(cell):
    """Without the cases that reach `cell`, the check above names it (and only cells those cases alone reached)."""
    rest = [c for c in cc.CASES if cell not in cc.cells_of(c)]
    assert len(rest) < len(cc.CASES)
    assert cell in cc.missing_cells(rest)


def test_route_mirror_at_the_boundaries():
    assert cc.critic_route(1, 64) == ("gen2", 4)
    assert [cc.critic_route(n, 64)[1] for n in (4, 5, 8, 9, 17, 18, 32)] == [4, 8, 8, 17, 17, 32, 32]
    assert cc.critic_route(33, 64) == ("gen1",)
    assert cc.critic_route(192, 64) == ("gen1",)
    assert cc.critic_route(193, 64) == ("wide",)
    assert cc.critic_route(5, 63) == ("generic",)
    assert cc.critic_route(156, 100) == ("generic",)
    assert cc.critic_route(157, 100) == ("wide",)
    assert {cc.critic_route(c[0], c[1])[0] for c in cc.CASES} == set(cc.ROUTES)


def test_cases_are_distinct_and_within_the_api():
    assert len({cc.case_id(c) for c in cc.CASES}) == len(cc.CASES)
    for n, F, T, Bc, head, _ in cc.CASES:
        assert 1 <= F <= 128 and 1 <= n <= 1024 and T >= 1 and Bc >= 1
        assert len(head) + 1 <= cc.MAX_LAYERS and all(1 <= w <= cc.THREADS for w in head)


@pytest.mark.parametrize("case", cc.CASES, ids=cc.case_id)
def test_case_inputs_stay_in_the_valid_range(case):
    pb, xseq, label, xs = cc.make_case(case)
    cr64 = orc.cast_problem(pb, np.float64)["critic"]
    if len(label) > 1:
        assert (label > 0).any() and (label < 0).any(), "mixed labels"
    for x in (xseq, xs):
        x64 = x.astype(np.float64)
        s = orc.critic_forward(cr64, x64)
        assert np.abs(s).max() < cc.SCORE_MAX, s
        assert not cc.head_kinks(cr64, x64).any(), "a head row sits at a relu kink: change the seed"
        assert cc.head_live_fraction(cr64, x64) >= 0.25, "the head closes for most rows: change the seed"


@pytest.mark.parametrize("n,F,head", [(1, 64, ()), (17, 7, (65, 3)), (5, 100, cc.DEEP)])
def test_split_critic_flat_follows_the_packing(n, F, head):
    import gpu_util as gu
    cr = _small_critic(n, F, head)
    flat = gu.critic_flat(dict(critic=cr))
    blocks = gu.split_critic_flat(flat, n, F, (F,) + head + (1,))
    want = [cr["Wx"], cr["Wh"], cr["b"]] + [a for W, b in cr["head"] for a in (W, b)]
    assert len(blocks) == len(want)
    for (_, got), w in zip(blocks, want):
        assert np.array_equal(got, w.reshape(-1))


def _small_critic(n, F, head):
    return orc.make_problem(n, 1, 2, 1, seed=3, dyn_hidden=(4,), cost_hidden=(4,), cost_fout=2, lstm_features=F,
                            head_hidden=head, bias_scale=0.1)["critic"]
