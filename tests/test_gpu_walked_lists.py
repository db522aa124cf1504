"""GPU tests of the lists the pair passes walk: the hit lists hit / hcnt / hlo and the row orders ord / ordu that upk_pairlist_refine and
upk_pairlist_order write from the cached lists once per force pass, the cached lists themselves, the rotamer graph's slot fields, and
the cached residue-pair list of backbone_pairs -- read with upside_hip_get_walked_lists / upside_hip_get_backbone_list (read only: no
kernel, no side built on demand) and checked pair by pair by tests/walked_lists.py, itself pinned on the CPU by
tests/test_walked_lists_cases.py.  upside_hip_get_pairlist, which the other parity tests use, filters the cached side-1 list with a
kernel of its own and so says nothing about these.

Every check runs in a child process with its own time limit (tests/walked_lists_gpu_worker.py, which prints each tally before it
asserts).  References: P.oracle_pairlist at the device's current positions for the five oracle-listed graphs, the all-pairs yardstick
on the device's source-node outputs for the radial graphs.  All comparisons are exact; no tolerance is involved."""
import os
import subprocess
import sys
import pytest

pytestmark = pytest.mark.gpu
WORKER = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'walked_lists_gpu_worker.py')
SWITCHES = ('UPSIDE_HIP_SKIN_SCALE', 'UPSIDE_HIP_GRAPH', 'UPSIDE_HIP_ASYNC_PREPARE', 'UPSIDE_HIP_BATCH', 'UPSIDE_HIP_PLB_UNSTAGED',
            'UPSIDE_HIP_BACKBONE_SKIN', 'UPSIDE_HIP_BACKBONE_LIST')


def run_check(which, tmp_path, timeout, args=(), env=None):
    child_env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    child_env.update(env or {})
    try:
        r = subprocess.run([sys.executable, WORKER, which, str(tmp_path)] + [str(a) for a in args], stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, timeout=timeout, env=child_env)
    except subprocess.TimeoutExpired as err:      # a hang: nothing more is started
        pytest.exit('check %s did not finish in %d s:\n%s' % (which, timeout, (err.stdout or b'').decode()[-3000:]), returncode=3)
    out = r.stdout.decode()
    print(out)
    if r.returncode not in (0, 1):      # killed by a signal or aborted: nothing more is started on a device that may have faulted
        pytest.exit('check %s ended with status %d:\n%s' % (which, r.returncode, out[-3000:]), returncode=3)
    assert r.returncode == 0, out[-6000:]
    assert 'CHECK %s PASSED' % which in out, out[-2000:]
    return out


def test_static_first_pass_of_fresh_engines(tmp_path):
    """one-system fresh engines, the first pass only: every fixture at pos and pos2, syn300_10A also compressed to 0.9 and stretched to
    1.3 about its centroid, proteinG56_7A to 0.5 and 2.0 (factors chosen on the CPU with the yardstick, see the worker).  Every property
    of check_graph for every graph and kept side, the row orders sorted by descending count; pooled over the structures the cached row
    lengths of the walked side-1 and side-2 lists must each fill the classes 0, 1..63, 65..128, > 128, and cnt % 64 in {0, 1, 63}"""
    run_check('static', tmp_path, 300)


@pytest.mark.parametrize('fixture,size', [('proteinG56_7A', '3'), ('proteinG56_7A', '16'), ('proteinG56_7A', '24'),
                                          ('trpcage20_7A', 'ncu+8'), ('trpcage20_7A', '2ncu+8')])
def test_md_script(tmp_path, fixture, size):
    """S systems at their own temperatures 0.5 .. 1.5 from the golden positions plus noise: run_steps(k) for k in 1, 5, 6, 7, 12, 13, 30,
    in between a derivative-only pass (flips the buffer parity against the captured graph), an energies-only call, set_system_pos of one
    system to a far structure, swap_systems and set_temperature; after every operation one compute, then check_graph on every graph of
    every system (S <= 24) or of the first, the last, every rebuilt and six quiet systems.  S in 3, 16, 24, n_cu + 8, 2 n_cu + 8: the
    planner's borders (skin, refine and build rows, upkeep block, merged launches, graph replay).  Per graph the check points must
    include one where no system, one where some and one where every system rebuilt"""
    run_check('md', tmp_path, 300, (fixture, size))


@pytest.mark.parametrize('size,switch', [('3', None), ('24', None), ('24', 'UPSIDE_HIP_GRAPH=0'), ('24', 'UPSIDE_HIP_ASYNC_PREPARE=0'),
                                         ('24', 'UPSIDE_HIP_BATCH=0'), ('24', 'UPSIDE_HIP_PLB_UNSTAGED=1')])
def test_tight_margin(tmp_path, size, switch):
    """the same script with UPSIDE_HIP_SKIN_SCALE=0.05: the cached list is barely larger than the in-range list, so any slack in the
    two-largest-displacements rule or a stale reference buffer loses a pair at once; at S = 24 also once each without graph replay,
    without the asynchronous list upkeep, without merged launches and with the unstaged list build.

    This case found a pair one ulp inside cache_cutoff missing from its cached row (S = 24, rotamer): dist2_exact was fused into an fma
    in the list build; the kernels are now compiled with truly rounded __fmul_rn / __fadd_rn / __fsub_rn (csrc/Makefile)"""
    env = {'UPSIDE_HIP_SKIN_SCALE': '0.05'}
    if switch:
        k, v = switch.split('=')
        env[k] = v
    run_check('md', tmp_path, 300, ('proteinG56_7A', size), env)


def test_radial_graphs(tmp_path):
    """radial and hbond_sc_radial (proteinG56_restraints, S = 3), which walk their cached lists and test the distance themselves: the same
    script; the walked pairs are the cached partners in range at cur_pos, the reference is the yardstick"""
    run_check('radial', tmp_path, 300)


@pytest.mark.parametrize('size,skin', [('3', None), ('24', None), ('3', '0.5'), ('24', '0.5')])
def test_backbone_list_and_its_bits(tmp_path, size, skin):
    """syn150_10A, 60 steps with the same interleaving, check_backbone after every operation (with the default skin and with
    UPSIDE_HIP_BACKBONE_SKIN=0.5); then a second child with UPSIDE_HIP_BACKBONE_LIST=0 evaluates the recorded positions and must return
    the same bits of the backbone_pairs potential for every system: the list only spares tests, it reorders no sum"""
    record = os.path.join(str(tmp_path), 'backbone_S%s.npz' % size)
    run_check('backbone', tmp_path, 300, (size, record), {'UPSIDE_HIP_BACKBONE_SKIN': skin} if skin else None)
    run_check('backbone_nolist', tmp_path, 300, (record,), {'UPSIDE_HIP_BACKBONE_LIST': '0'})


def test_refusals_state_their_reason_and_leave_the_engine_usable(tmp_path):
    """a side that is not kept, side 2 of a symmetric graph, a node without a graph, a bad system index, too small a buffer, the backbone
    accessor with the list off: each states its reason; two reads agree and a compute afterwards returns the bits of the one before"""
    run_check('refusals', tmp_path, 300)
