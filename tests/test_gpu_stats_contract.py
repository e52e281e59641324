"""What every entry point writes into wos_stats (include/wos.h), against a fixture recorded from
the parent of the change that split the C ABI host code by concern (csrc/wos_capi_*.cpp).  The
parity tests look at outputs only; a slip in the enqueue protocol those units share (a slot left
with another solve's shape, counters read from the wrong workspace, a ticket not handed out)
leaves the outputs right and shows only here.

Compared per call (tests/stats_contract.py lists the calls): the nine counters, walk_launches,
first_ball_blocks_per_cu, walk_blocks_per_cu, walk_lds_bytes, star_grid, geom_global, dir_grid,
whether ticket is zero, and which of kernel_ms / first_ball_ms / walk_ms / fold_ms are zero.

70 points of 6 walks cannot be split into two batches: wos_set_max_batch_tasks clamps the cap
to 2^16 tasks.  So every call runs twice, with 6 walks (one batch) and with 1024 walks, where
the same cap splits the same 70 points into 64 + 6.

tests/golden/stats_contract.json is written by `python tests/stats_contract.py --write` with
WOS_LIB_PATH naming the parent commit's library (the fixture records that commit), never by the
code under test."""
import json

import pytest

import stats_contract

pytestmark = pytest.mark.gpu

with open(stats_contract.FIXTURE) as _f:
    GOLDEN = json.load(_f)


@pytest.fixture(scope="module")
def measured(gpu):
    return stats_contract.collect()


def test_the_fixture_describes_these_calls(measured):
    assert (GOLDEN["n_points"], GOLDEN["walks"], GOLDEN["batch_cap"]) == (
        stats_contract.N_POINTS, list(stats_contract.WALKS), stats_contract.BATCH_CAP)
    assert len(GOLDEN["parent_commit"]) == 40
    assert sorted(measured) == sorted(GOLDEN["calls"])
    # the cases are what the docstring says: one batch of 6 walks, two batches of 1024
    assert GOLDEN["calls"]["w6/solve_host"]["walk_launches"] == 1
    assert GOLDEN["calls"]["w1024/solve_host"]["walk_launches"] == 2
    assert GOLDEN["calls"]["w1024/tape_record"]["walk_launches"] == 4
    assert GOLDEN["calls"]["w6/solve_host"]["points_estimated"] == stats_contract.N_POINTS - 1  # one point outside


@pytest.mark.parametrize("call", sorted(GOLDEN["calls"]))
def test_stats_match_the_parent(measured, call):
    got, want = measured[call], GOLDEN["calls"][call]
    print(call, got)
    assert got == want, {k: (got[k], want[k]) for k in want if got.get(k) != want[k]}
