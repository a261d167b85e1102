"""What mugiq_hip_loop_plan reports is what mugiq_hip_loop_compute does: one spawned rank with z and t partitioned as its own
neighbour (mp_workers.plan_worker), the plan asked for before the compute and compared with the entry kernels, the phases and the
pool allocations of the compute, and the results with the single-domain oracle."""
import pytest
import torch.multiprocessing as mp

import mp_workers
from test_multi_rank_cpu import free_port

pytestmark = pytest.mark.gpu


# scratch_alloc byte counts inside the first and the second compute, as measured at commit 598c0d4 (before the plan was made in
# one place): host logic, so the lists must be equal, not close
@pytest.mark.parametrize("G,case,alloc_first,alloc_second", [
    ((8, 16, 8, 8), "pack", [1253376], []),
    ((4, 4, 8, 8), "pool_tie", [221184], [65536])])
def test_compute_follows_the_plan(G, case, alloc_first, alloc_second):
    mp.spawn(mp_workers.plan_worker, args=(1, free_port(), G, case, alloc_first, alloc_second), nprocs=1, join=True)
