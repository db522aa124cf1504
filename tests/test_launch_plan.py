"""The launch policy (upside-md_amd/csrc/launch_plan.h) asked without a GPU: launch_plan_host.cpp, a stand-alone program compiled here, prints
the plan for given numbers and hand-filled switches; the anchors below are derived by hand from the thresholds and LDS formulas."""
import os
import subprocess
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
PAIR_LDS = 158 * 1024


@pytest.fixture(scope='module')
def plan(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('launch_plan') / 'launch_plan_host')
    subprocess.run(['g++', '-O1', '-std=c++17', '-Wall', '-o', exe, os.path.join(HERE, 'launch_plan_host.cpp')], check=True)

    def run(query, env=None, **kw):
        out = subprocess.run([exe, query] + ['%s=%s' % kv for kv in kw.items()], check=True, stdout=subprocess.PIPE, env=env).stdout.decode()
        rows = [line.split('=', 1) for line in out.splitlines() if '=' in line and not line.startswith('violation:')]
        r = {k: float(v) for k, v in rows}
        r['violations_text'] = [line for line in out.splitlines() if line.startswith('violation:')]
        return r
    return run


def test_merged_launches_and_graph(plan):
    for S, n_atom, on in ((1, 900, 1), (16, 5000, 1), (17, 5000, 0), (26, 900, 1), (27, 900, 0), (142, 168, 1), (143, 168, 0), (160, 60, 1), (161, 60, 0)):
        r = plan('engine', S=S, n_atom=n_atom)
        assert r['merged'] == on and r['graph'] == on, (S, n_atom)
        assert plan('engine', S=S, n_atom=n_atom, trace=1)['graph'] == 0
        for force in (0, 1):
            f = plan('engine', S=S, n_atom=n_atom, BATCH=force)
            assert f['merged'] == force and f['graph'] == force
            assert plan('engine', S=S, n_atom=n_atom, GRAPH=force)['graph'] == force
            assert plan('engine', S=S, n_atom=n_atom, GRAPH=force, trace=1)['graph'] == 0


def test_fused_list_lanes(plan):
    for S, lanes in ((255, 1024), (256, 512), (2047, 512), (2048, 256)):
        r = plan('engine', S=S)
        assert r['lanes'] == lanes and r['lanes_heavy'] == min(lanes, 512)
    for S in (1, 4096):
        assert plan('engine', S=S, FUSE_THREADS=128)['lanes'] == 128 and plan('engine', S=S, FUSE_THREADS=128)['lanes_heavy'] == 128
        for ignored in (100, 2048):
            assert plan('engine', S=S, FUSE_THREADS=ignored)['lanes'] == plan('engine', S=S)['lanes']
    assert plan('engine', S=255, n=64)['heavy_alone'] == 0 and plan('engine', S=256, n=64)['heavy_alone'] == 1 and plan('engine', S=1, n=65)['heavy_alone'] == 1


def test_pair_graph_thresholds(plan):
    for S, other, side_chain in ((16, 1.5, 1.5), (17, 0.5, 0.5), (256, 0.5, 0.5), (257, 0.75, 0.5)):
        r = plan('graph', S=S)
        assert (r['skin'], r['skin_side_chain']) == (other, side_chain)
        r = plan('graph', S=S, SKIN_SCALE=1.0)
        assert (r['skin'], r['skin_side_chain']) == (1.0, 1.0)
    assert plan('graph', S=255)['gacc'] == 1 and plan('graph', S=256)['gacc'] == 0 and plan('graph', S=1)['gacc_symmetric'] == 0
    # upkeep kernels against the CU count
    assert plan('graph', S=511, n_cu=256)['upkeep_block'] == 1024 and plan('graph', S=512, n_cu=256)['upkeep_block'] == 256
    assert plan('graph', S=255, n_cu=256)['list_build_rows'] == 64 and plan('graph', S=256, n_cu=256)['list_build_rows'] == 128
    for S, n_rows, rows in ((15, 1000, 16), (16, 1000, 64), (255, 1000, 64), (256, 1000, 256), (256, 512, 128), (256, 513, 256)):
        assert plan('graph', S=S, n_cu=256, n_rows=n_rows)['refine_rows'] == rows


def test_pair_geometry(plan):
    for S, rows, lanes_per_row, per_wg, bps, lanes in ((4096, 1000, 4, 256, 1, 1024), (1, 1000, 8, 128, 8, 1024), (1, 1000, 4, 256, 4, 1024), (64, 300, 8, 128, 3, 832)):
        r = plan('geometry', S=S, rows=rows, lanes_per_row=lanes_per_row, rows_per_full_wg=per_wg)
        assert (r['wgs_per_system'], r['lanes']) == (bps, lanes)
    # IG_WGS < 1 means 256
    assert plan('geometry', S=1, rows=1000, lanes_per_row=8, rows_per_full_wg=128, IG_WGS=0)['wgs_per_system'] == 8
    assert plan('geometry', S=1, rows=1000, lanes_per_row=8, rows_per_full_wg=128, IG_WGS=2)['wgs_per_system'] == 2


def test_coverage_pair_passes(plan):
    """hbond_coverage of a 300-residue protein (n_param 40, 132 polynomial floats per type pair): the polynomial table and the packed passes; a
    table of words (tab + 3 & ~3) + 8 (n1 + n2) + n_max + (n_max + 1) / 2 + 4"""
    g = dict(coverage=1, has_poly=1, n1=600, n2=1000, cap1=512, cap2=512, n_type1=2, n_type2=20, n_param=40, n_poly=132, side=1, mode=0, d_other=6)
    base = (40 * 132 + 8 * 1600 + 1000 + 500 + 4) * 4
    r = plan('pair', **g)
    assert r['table'] == 2 and r['tab_floats'] == 5280 and r['lds_bytes'] == base
    assert r['fwd.packed'] == 1 and r['fwd.lds_bytes'] == base + 64
    assert r['bwd.packed'] == 1 and r['bwd.lds_bytes'] == base + 8 + 1000 * 6 * 8 + 64 + 600 * 4 and r['passes_staged'] == 1
    r = plan('pair', PAIR2=0, **g)
    assert r['fwd.packed'] == 0 and r['fwd.lds_bytes'] == base and r['bwd.packed'] == 0 and r['bwd.lds_bytes'] == base + 8 + 1000 * 6 * 8
    r = plan('pair', IG_POLY=0, **g)
    assert r['table'] == 1 and r['tab_floats'] == 1600
    r = plan('pair', IG_UNSTAGED=1, **g)
    assert r['table'] == 0 and r['fwd.table'] == 0 and r['bwd.table'] == 0 and r['passes_staged'] == 0
    assert plan('pair', **dict(g, cap1=65536))['table'] == 0
    assert plan('pair', **dict(g, coverage=0, has_poly=0))['table'] == 1          # other graphs: never the polynomial table, never packed
    assert plan('pair', **dict(g, coverage=0, has_poly=0))['fwd.packed'] == 0
    # the polynomial table fits alone (38084 words) but not beside the 14408 bytes of accumulators: the backward pass falls to the coefficients
    # (3680 words less), which in turn leave no room for the packed pass's 64 + 4 n1 bytes
    big = dict(g, n1=3200, n2=300)
    r = plan('pair', **big)
    assert r['table'] == 2 and r['lds_bytes'] == 38084 * 4 and r['fwd.packed'] == 1
    assert (r['bwd.table'], r['bwd.packed'], r['bwd.lds_bytes']) == (1, 0, 34404 * 4 + 14408)
    for r in (plan('pair', **g), plan('pair', **big)):
        assert r['fwd.lds_bytes'] <= PAIR_LDS and r['bwd.lds_bytes'] <= PAIR_LDS


def test_solve_capacities_and_thresholds(plan):
    assert plan('solve', S=511, n_node=300)['layout_record'] == 0 and plan('solve', S=512, n_node=300)['layout_record'] == 1
    assert plan('solve', S=4096, n_node=300, BP_LAYOUT=0)['layout_record'] == 0
    assert plan('solve', S=1, n_node=300, BP_LAYOUT=1)['layout_record'] == 1 and plan('solve', S=1, n_node=300, BP_LAYOUT=2)['layout_record'] == 1
    for S, n_node, K in ((256, 65, 4), (256, 64, 1), (257, 300, 1)):
        assert plan('solve', S=S, n_node=n_node)['slot_split'] == K
    for S, n_node in ((1, 20), (257, 300), (4096, 65)):
        assert plan('solve', S=S, n_node=n_node, SLOT_SPLIT=3)['slot_split'] == 3
    r = plan('solve', n_node=300)
    assert r['slot_cap'] == 28800 and r['adj_cap'] == 256
    assert plan('solve', n_node=20)['slot_cap'] == 190 and plan('solve', n_node=20)['adj_cap'] == 20 and plan('solve', n_node=1)['slot_cap'] == 1
    assert plan('solve', n_node=300, SLOT_FACTOR=8, ADJ_CAP=16)['slot_cap'] == 2400 and plan('solve', n_node=300, ADJ_CAP=16)['adj_cap'] == 16


def test_cluster_size(plan):
    big = dict(n_cu=256, n_node=300, n_node1=0, need=200000, widest=3000)      # 35688 floats per workgroup: ceil(230000 / 35688) = 7 = ceil(3450 / 512)
    for S in (1, 24, 25):
        assert plan('solve', S=S, **big)['C'] == 7                              # 256 / 7 = 36 -> 32 systems per launch, 4/5 of it = 25
    assert plan('solve', S=26, **big)['C'] == 1 and plan('solve', S=4096, **big)['C'] == 1
    assert plan('solve', S=4096, BP_CLUSTER=7, **big)['C'] == 7 and plan('solve', S=1, BP_CLUSTER=1, **big)['C'] == 1
    r = plan('solve', S=25, n=5, **big)
    assert r['per_launch'] == 32 and r['grid_x'] == 8
    assert plan('solve', S=1, **dict(big, n_node1=294))['C'] == 1               # fewer multi-state nodes than workgroups
    assert plan('solve', S=1, **dict(big, need=600000))['C'] == 1               # C = 20 > 16
    for S in (1, 8, 4096):
        assert plan('solve', S=S, **dict(big, need=80000, widest=500))['C'] == 1    # C = 3: below the C >= 6 rule at any batch size
    assert plan('solve', S=1, BP_CLUSTER=3, **dict(big, need=80000, widest=500))['C'] == 3


def test_matrix_form(plan):
    for C in (1, 7):
        for one_bead in (0, 1):
            for table in (0, 1):
                f = plan('form', S=1, merged=1, C=C, one_bead=one_bead, BP_ENERGY_TABLE=table)
                assert f['p_prob'] == (1 if C == 1 and one_bead and not table else 0)
    for S, merged, on in ((16, 0, 1), (17, 0, 0), (17, 1, 1), (4096, 0, 0)):
        assert plan('form', S=S, merged=merged, C=1, one_bead=1)['node_prob_in_solve'] == on
        assert plan('form', S=S, merged=merged, C=1, one_bead=1, NODE_PROB_IN_SOLVE=0)['node_prob_in_solve'] == 0
    for layout_record in (0, 1):
        for in_solve in (0, 1):             # S = 4096 unmerged: node_prob_in_solve follows the switch only through S <= 16 or merged
            for p_prob in (0, 1):
                f = plan('form', S=16 if in_solve else 4096, merged=0, C=1, one_bead=p_prob, layout_record=layout_record)
                assert (f['node_prob_in_solve'], f['p_prob']) == (in_solve, p_prob)
                assert f['prefold'] == (1 if layout_record and not in_solve and p_prob else 0)


def test_one_workgroup_solve(plan):
    r = plan('bp', n_node=300, slot_cap=28800, layout_record=1)
    assert r['refused'] == 0 and r['lds_base'] == 17088 and r['msg_bytes'] == 146752 and r['msg_floats'] == 36688
    assert r['dense'] == 1 and r['scratch_words'] == 910 and r['layout_lds'] == 12444 and r['layout_launch'] == 1
    assert plan('bp', n_node=300, slot_cap=28800, layout_record=0)['layout_launch'] == 0
    r = plan('bp', n_node=300, slot_cap=28800, layout_record=1, BP_LDS_MSG_KB=0)
    assert r['msg_bytes'] == 0 and r['dense'] == 0 and r['layout_launch'] == 0
    assert plan('bp', n_node=300, slot_cap=28800, layout_record=1, BP_COMPACT=0)['dense'] == 0
    assert plan('bp', n_node=300, slot_cap=28800, layout_record=1, have_rows=0)['dense'] == 0
    assert plan('bp', n_node=300, slot_cap=28800, layout_record=1, BP_LAYOUT=2)['scratch_words'] == 1
    # the message inbox never exceeds 64 bytes per slot; (14 n + 72) words of node arrays past 155 KB are refused (9004)
    assert plan('bp', n_node=20, slot_cap=190)['msg_bytes'] == 190 * 64
    assert plan('bp', n_node=2829, slot_cap=100000)['refused'] == 0 and plan('bp', n_node=2830, slot_cap=100000)['refused'] == 1
    # a layout record whose launch would need more than a quarter of a CU's LDS: laid out inside the solve
    # (7 n + 85 words of node rows, 2 words per 32 of 2 (slot_cap / 4 + 32) + 64 rows + 2, 64 bytes: 40 KB lie between these two capacities)
    r = plan('bp', n_node=1024, slot_cap=94783, layout_record=1)
    assert r['dense'] == 1 and r['scratch_words'] == 2970 and r['layout_lds'] == 7253 * 4 + 2970 * 4 + 64 and r['layout_launch'] == 1
    r = plan('bp', n_node=1024, slot_cap=94784, layout_record=1)
    assert r['dense'] == 1 and r['scratch_words'] == 2972 and r['layout_lds'] == 40964 and r['layout_launch'] == 0


LIB = dict(n_type=20, n_param=40, n_poly=132)          # 210 type pairs: 8400 coefficient floats, 27720 polynomial floats


def test_side_chain_pair_passes(plan):
    r = plan('rot', S=4096, n_bead=1000, **LIB)
    assert r['bead_pack'] == 0
    assert (r['energy.fits'], r['energy.poly'], r['energy.staged'], r['energy.packed']) == (1, 1, 1, 0)
    assert r['energy.lds_bytes'] == 148896 and r['energy.tab_floats'] == 27720 and (r['energy.grid_x'], r['energy.lanes']) == (1, 1024)
    assert (r['grad.fits'], r['grad.packed'], r['grad.poly'], r['grad.staged']) == (1, 1, 0, 1)
    assert r['grad.lds_bytes'] == 119648 and r['grad.tab_floats'] == 8400
    assert (27720 + 1504) * 4 + 80000 + 32 == 196928 > PAIR_LDS and r['grad_poly_packed_staged'] == 0      # the polynomial table beside the accumulators
    assert (r['grad.grid_x'], r['grad.lanes']) == (1, 1024)
    r = plan('rot', S=1, n_bead=1000, **LIB)
    assert (r['energy.grid_x'], r['energy.lanes'], r['grad.grid_x'], r['grad.lanes']) == (8, 1024, 4, 1024)
    # a small library's polynomial table fits the packed gradient pass too
    r = plan('rot', S=64, n_bead=300, **LIB)
    assert (r['grad.packed'], r['grad.poly'], r['grad.tab_floats']) == (1, 1, 27720)
    r = plan('rot', S=4096, n_bead=1000, PAIR2=0, **LIB)
    assert (r['grad.fits'], r['grad.packed'], r['grad.poly'], r['grad.staged']) == (1, 0, 0, 1) and r['grad.lds_bytes'] == 119616
    r = plan('rot', S=4096, n_bead=1000, ROT_POLY=0, **LIB)
    assert (r['energy.poly'], r['energy.staged'], r['energy.tab_floats']) == (0, 1, 8400)
    r = plan('rot', S=4096, n_bead=1000, ROT_UNSTAGED=1, **LIB)
    assert r['bead_pack'] == 1
    for p in ('energy', 'grad'):
        assert (r[p + '.fits'], r[p + '.staged'], r[p + '.packed'], r[p + '.poly']) == (1, 0, 0, 0) and r[p + '.lds_bytes'] == (8400 + 1500 + 4) * 4


def test_bead_pack_bound_decides_where_the_exact_formula_still_fits(plan):
    """8400 + 22 n + 8 words first exceed 158 KB at n = 1457, where the scalar gradient pass itself needs 8400 + 21.5 n + 4.5: the rows are
    allocated, and a system that has them uses them in both passes"""
    r = plan('rot', S=4096, n_bead=1456, **LIB)
    assert r['bead_pack'] == 0 and r['grad.staged'] == 1 and r['energy.staged'] == 1
    r = plan('rot', S=4096, n_bead=1457, **LIB)
    assert r['grad_scalar_exact_bytes'] == (8400 + 1457 + 729 + 4 + 20 * 1457) * 4 <= PAIR_LDS
    assert r['bead_pack'] == 1
    for p in ('energy', 'grad'):
        assert (r[p + '.fits'], r[p + '.staged'], r[p + '.packed']) == (1, 0, 0)


def test_table_too_large_for_lds(plan):
    r = plan('rot', S=1, n_bead=1000, n_type=60, n_param=62, n_poly=260)          # 1830 type pairs x 62 floats = 443 KB
    assert r['energy.fits'] == 0 and r['grad.fits'] == 0


def test_side_chain_pass_sweep_is_self_consistent(plan):
    r = plan('sweep')
    assert r['cases'] == 8 * 3 * 8191
    assert r['violations'] == 0, r['violations_text']


def test_switches_come_from_the_environment(plan):
    clean = {k: v for k, v in os.environ.items() if not k.startswith('UPSIDE_HIP_')}
    r = plan('env', env=clean)
    assert r['BATCH'] == -2 ** 31 and r['GRAPH'] == -1 and r['SLOT_FACTOR'] == 96 and r['BP_LAYOUT'] == -1 and r['BP_LDS_MSG_KB'] == 160
    assert r['IG_WGS'] == 256 and r['NBR_CAP'] == 512 and r['BACKBONE_SKIN'] == 3 and r['SKIN_SCALE'] == 0 and r['PAIR2'] == 1
    r = plan('env', env=dict(clean, UPSIDE_HIP_BATCH='0', UPSIDE_HIP_SLOT_FACTOR='12.5', UPSIDE_HIP_BP_LAYOUT='2', UPSIDE_HIP_PAIR2='0',
                             UPSIDE_HIP_BACKBONE_LIST_CAP='64', UPSIDE_HIP_SKIN_SCALE='0.6'))
    assert r['BATCH'] == 0 and r['SLOT_FACTOR'] == 12.5 and r['BP_LAYOUT'] == 2 and r['PAIR2'] == 0 and r['BACKBONE_LIST_CAP'] == 64
    assert abs(r['SKIN_SCALE'] - 0.6) < 1e-6 and r['GRAPH'] == -1
