"""GPU (-m gpu): the population forms of the no-wait optimiser launches (gemm_batch_pop_kernel<1, 1, 4>, adam_pop_kernel,
adam_pair_pop_kernel).  Where the fused optimiser launch is not admitted — at the headline shapes with four members the whole
population grid does not fit the device at once, and with meetings off it is never used — a population step must still issue
EVERY recorded launch position as one population launch (gcrl_pop_launch_counts: nothing member by member), and stay bitwise
equal to standalone agents."""
import numpy as np
import pytest

import test_gpu_population as ddpg_t
import test_gpu_population_td3 as td3_t

pytestmark = pytest.mark.gpu

SHAPES = {"cfg1": (10, 3, 64), "headline": (23, 4, 256)}   # (S, A, H) at B = 256


def _ddpg_pop(gcrl, shape, P, seeds):
    S, A, H = SHAPES[shape]
    return ddpg_t._pop(gcrl, S, A, ddpg_t._cfgs(P, H, 256), 40, seeds)


def test_ddpg_headline_p4_all_merged(gcrl):
    pop = _ddpg_pop(gcrl, "headline", 4, [11, 12, 13, 14])
    assert pop.launch_counts() == (0, 0)
    pop.update_many(1, 40)      # steps 1..40: the overlapped schedule, a Polyak step at its end
    merged, alone = pop.launch_counts()
    assert alone == 0 and merged > 0, (merged, alone)
    pop.update_many(41, 40)
    merged2, alone2 = pop.launch_counts()
    assert alone2 == 0 and merged2 > merged, (merged2, alone2)


def test_td3_h256_p4_all_merged(gcrl):
    S, A = 23, 4
    pop = td3_t._pop(gcrl, S, A, td3_t._cfgs(4, 256, 256), 40, [15, 16, 17, 18])
    pop.update_many(1, 40)      # actor steps and critic-only steps (ac_update_freq = 2)
    merged, alone = pop.launch_counts()
    assert alone == 0 and merged > 0, (merged, alone)


def test_single_member_issues_alone(gcrl):
    pop = _ddpg_pop(gcrl, "cfg1", 1, [19])
    pop.update_many(1, 8)
    merged, alone = pop.launch_counts()
    assert merged == 0 and alone > 0, (merged, alone)


@pytest.mark.parametrize("shape", ["cfg1", "headline"])
def test_ddpg_meetings_off_p4_bitwise(gcrl, shape):
    """meetings off: the members record the two-launch optimiser (GEMM batch + paired Adam), which now merges"""
    S, A, H = SHAPES[shape]
    seeds = [21, 22, 23, 24]
    pop, solo = ddpg_t._pair(gcrl, S, A, ddpg_t._cfgs(4, H, 256), 40, seeds)
    for ag in list(pop.members) + solo:
        ag.set_meetings(False)
    assert all(m.meetings() & (2 | 8) == 0 for m in pop.members)
    ddpg_t._run_and_compare(pop, solo, [(1, 40), (41, 40)])
    merged, alone = pop.launch_counts()
    assert alone == 0 and merged > 0, (merged, alone)
