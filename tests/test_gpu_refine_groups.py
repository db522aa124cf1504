"""GPU tests of the list refine's lane groups (csrc/kernels_igraph.hip d_pairlist_refine: LPR lanes per row, 64 / LPR rows per wavefront
trip): the hit lists hit / hcnt / hlo, read with Ensemble.walked_lists and checked word for word by walked_lists.check_graph against the
oracle's pair lists, at the row lengths and row counts where the kernel's trips and sets change.  Every check runs in a child process
with its own time limit (tests/refine_groups_gpu_worker.py, which prints each tally before it asserts); after a signal or a timeout
nothing more is started.  All comparisons are exact."""
import os
import subprocess
import sys
import pytest

pytestmark = pytest.mark.gpu
WORKER = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'refine_groups_gpu_worker.py')
SWITCHES = ('UPSIDE_HIP_SKIN_SCALE', 'UPSIDE_HIP_GRAPH', 'UPSIDE_HIP_ASYNC_PREPARE', 'UPSIDE_HIP_BATCH', 'UPSIDE_HIP_PLB_UNSTAGED')


def run_check(which, timeout, args=(), env=None):
    child_env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    child_env.update(env or {})
    try:
        r = subprocess.run([sys.executable, WORKER, which] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                           timeout=timeout, env=child_env)
    except subprocess.TimeoutExpired as err:      # a hang: nothing more is started
        pytest.exit('check %s did not finish in %d s:\n%s' % (which, timeout, (err.stdout or b'').decode()[-3000:]), returncode=3)
    out = r.stdout.decode()
    print(out)
    if r.returncode not in (0, 1):      # killed by a signal or aborted: nothing more is started on a device that may have faulted
        pytest.exit('check %s ended with status %d:\n%s' % (which, r.returncode, out[-3000:]), returncode=3)
    assert r.returncode == 0, out[-6000:]
    assert 'CHECK %s PASSED' % which in out, out[-2000:]


@pytest.mark.parametrize('size', ['1', '3'])
def test_first_pass_of_fresh_engines(size):
    """fresh engines of S systems, the first pass: edge_gly5 (5 rows per side: fewer rows than a wavefront has groups, and empty rows),
    trpcage20_7A, and proteinG56_7A as shipped, compressed to 0.5 and stretched to 2.0 about its centroid.  check_graph on every graph
    and kept side of every system.  Pooled over the structures, the cached rows of the 16-bit lists and of the 32-bit list must each fill
    the classes 0, 1..LPR-1, LPR, LPR+1..2 LPR, > 2 LPR and cnt % LPR in {0, 1, LPR-1} for the LPR their instance was compiled with, and
    one graph's row count must be a multiple neither of the rows of a set nor of a wavefront's run (211 bead rows, 5 rows)"""
    run_check('static', 120, (size,))


def test_first_pass_without_merged_launches():
    """the same at S = 3 with UPSIDE_HIP_BATCH=0: the refine's own launches (256-lane workgroups) instead of the merged ones"""
    run_check('static', 120, ('3',), {'UPSIDE_HIP_BATCH': '0'})


def test_four_sets_per_wavefront():
    """proteinG56_7A, its three structures, at S = 17: 64 rows per workgroup, so a wavefront walks four sets and the last wavefront of
    211 rows a ragged one"""
    run_check('static', 120, ('17',))


def test_some_systems_rebuild_past_the_cu_count():
    """trpcage20_7A, S = n_cu + 8 at temperatures 0.5 .. 1.5: 256 rows per workgroup; checks after the first pass and after 1, 5, 6 and 7
    more steps, on the first, the last, three rebuilt and three quiet systems per graph; at some check point some systems must have
    rebuilt a list and some not"""
    run_check('md', 180, ('ncu+8',))
