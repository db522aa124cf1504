"""Perturbed parameter tables for the set_param tests (test_set_param_cases.py on the oracle, test_gpu_set_param.py on the device):
a case names a fixture and, per node, how its table is perturbed; build() writes the perturbed tables into a copy of the fixture and
returns them as the engine must serve them (the file's values cast to f4, flat, in file order).

The tables keep what update_cutoffs / is_compatible demand of them: the side-chain table is drawn per unordered type pair, its
mirror entry [b, a] is [a, b] with the two angular halves exchanged and the radial part equal, and on the diagonal the two angular
halves agree.  The directions of the fixed placements stay unit vectors.  The cut-off of environment_coverage (p[0] + 1 / p[1]) moves by the shift of p[0]; that of hbond_sc_radial
((14 - 1e-6) / p[0]) grows by 1 / 0.8."""
import gc
import numpy as np
import parity_util as P
import hamiltonian_files as H

# node -> (group below /input/potential that holds the table, dataset)
TABLES = {
    'rotamer': ('rotamer/pair_interaction', 'interaction_param'),
    'hbond_coverage': ('hbond_coverage', 'interaction_param'),
    'hbond_coverage_hydrophobe': ('hbond_coverage_hydrophobe', 'interaction_param'),
    'environment_coverage': ('environment_coverage', 'interaction_param'),
    'protein_hbond': ('protein_hbond', 'interaction_param'),
    'hbond_sc_radial': ('hbond_sc_radial', 'interaction_param'),
    'placement_fixed_point_vector_only': ('placement_fixed_point_vector_only', 'placement_data'),
    'placement_fixed_point_vector_only_CB': ('placement_fixed_point_vector_only_CB', 'placement_data'),
    'placement_fixed_point_vector_scalar': ('placement_fixed_point_vector_scalar', 'placement_data'),
    'placement_fixed_point_only_CB': ('placement_fixed_point_only_CB', 'placement_data'),
    'nonlinear_coupling_environment': ('nonlinear_coupling_environment', 'coeff'),
    'linear_coupling_uniform_env': ('linear_coupling_uniform_env', 'couplings'),
    'linear_coupling_with_inactivation_env': ('linear_coupling_with_inactivation_env', 'couplings'),
}
# the nodes whose set_param the oracle serves (the interaction graphs with a table of their own)
ORACLE_SETTABLE = ('rotamer', 'hbond_coverage', 'hbond_coverage_hydrophobe', 'environment_coverage', 'hbond_sc_radial')
# the five graphs whose canonical pair lists both engines serve
PAIRLIST_NODES = ('rotamer', 'hbond_coverage', 'hbond_coverage_hydrophobe', 'environment_coverage', 'protein_hbond')
# the nodes with a get_param_deriv on both engines, and its bound (test_param_derivs_match_reference_golden)
NO_PARAM_DERIV = ('protein_hbond',)


def param_deriv_tol(node):
    return 5e-5 if node.startswith('placement') else 1e-5


_ROTAMER_KNOTS = {34: 9, 40: 12, 62: 16}      # n_param -> radial knots (IGraphHost: n_param = 2 n_knot_angular + 2 n_knot)


def side_chain_table(T, rs, amp=0.2):
    nt, nt2, n_param = T.shape
    assert nt == nt2
    na = (n_param - 2 * _ROTAMER_KNOTS[n_param]) // 2
    N = T.copy()
    for a in range(nt):
        for b in range(a, nt):
            f = 1. + amp * rs.uniform(-1, 1, n_param)
            if a == b:
                f[na:2 * na] = f[:na]
            N[a, b] = T[a, b] * f
            m = N[a, b].copy()
            m[:na] = N[a, b][na:2 * na]
            m[na:2 * na] = N[a, b][:na]
            N[b, a] = m
    return N


def scaled(T, rs, amp=0.2):
    return T * (1. + amp * rs.uniform(-1, 1, T.shape))


def noisy(T, rs, amp=0.1):
    """a fixed placement's rows [point | direction | scalar] plus uniform noise; the directions (columns 3:6) are brought back to unit
    length, because the angular splines of the pair functors are defined for cosines in [-1, 1] only and are not clamped
    (bead_interaction.h:46-53): a longer direction reads past the end of its table, in the reference as in every engine"""
    N = T + amp * rs.uniform(-1, 1, T.shape)
    if N.shape[-1] >= 6:
        N[..., 3:6] /= np.sqrt((N[..., 3:6] ** 2).sum(axis=-1, keepdims=True))
    return N


def environment_shift(T, rs, shift=1.0):
    T = T.copy()
    T[..., 0] += shift
    return T


def radial_table(T, rs, p0_scale=0.8, amp=0.2):
    T = T.copy()
    T[..., 0] *= p0_scale
    T[..., 1:] *= 1. + amp * rs.uniform(-1, 1, T[..., 1:].shape)
    return T


def protein_hbond_table(T, rs):
    """[inner radius, its sharpness, outer radius, its sharpness, angular threshold, its sharpness, ...]: the radii move inwards and the
    sigmoids soften, so that every bond that scores stays within the graph's fixed 3.5 A cut-off"""
    T = T.copy()
    T[..., 0] += 0.10
    T[..., 2] -= 0.15
    T[..., 1] *= 0.85
    T[..., 3] *= 1.15
    T[..., 4] -= 0.05
    T[..., 5] *= 0.9
    return T


def _p(fn, **kw):
    return (fn, kw)


ALL_7A = [('rotamer', _p(side_chain_table)), ('environment_coverage', _p(environment_shift, shift=1.0)),
          ('hbond_coverage', _p(scaled)), ('hbond_coverage_hydrophobe', _p(scaled))]
ALL_RESTRAINTS = [('hbond_sc_radial', _p(radial_table)), ('placement_fixed_point_only_CB', _p(noisy, amp=0.3)),
                  ('placement_fixed_point_vector_only', _p(noisy, amp=0.1)), ('nonlinear_coupling_environment', _p(scaled, amp=0.3)),
                  ('linear_coupling_uniform_env', _p(scaled, amp=0.3)), ('linear_coupling_with_inactivation_env', _p(scaled, amp=0.3)),
                  ('environment_coverage', _p(environment_shift, shift=-1.5))]
# ... and every other settable table of the 7 A force field behind them (the first four draw what ALL_7A draws)
EVERY_7A = ALL_7A + [('protein_hbond', _p(protein_hbond_table)), ('nonlinear_coupling_environment', _p(scaled, amp=0.3)),
                     ('placement_fixed_point_vector_only', _p(noisy, amp=0.1)), ('placement_fixed_point_vector_only_CB', _p(noisy, amp=0.3)),
                     ('placement_fixed_point_vector_scalar', _p(noisy, amp=0.2))]

# case id -> (fixture, seed, [(node, (perturbation, keywords))]).  The 'all_*' cases move the
# side-chain, coverage and environment tables together (restraints: the tables only that fixture has); 'every_*' adds the rest.
CASES = {
    'every_proteinG56_7A': ('proteinG56_7A', 1, EVERY_7A),
    'every_syn150_10A': ('syn150_10A', 1, EVERY_7A),
    'md_proteinG56_7A': ('proteinG56_7A', 1, ALL_7A[:2]),      # side chains and environment_coverage (the cut-off grows by 1 A)
    'all_trpcage20_7A': ('trpcage20_7A', 1, ALL_7A),
    'all_proteinG56_7A': ('proteinG56_7A', 1, ALL_7A),
    'all_syn150_10A': ('syn150_10A', 1, ALL_7A),
    'all_proteinG56_restraints': ('proteinG56_restraints', 2, ALL_RESTRAINTS),
    # one node at a time
    'rotamer': ('trpcage20_7A', 1, [('rotamer', _p(side_chain_table))]),
    'hbond_coverage': ('trpcage20_7A', 1, [('hbond_coverage', _p(scaled, amp=0.3))]),
    'hbond_coverage_hydrophobe': ('trpcage20_7A', 1, [('hbond_coverage_hydrophobe', _p(scaled, amp=0.3))]),
    'environment_coverage_grow': ('trpcage20_7A', 1, [('environment_coverage', _p(environment_shift, shift=1.0))]),
    'environment_coverage_shrink': ('trpcage20_7A', 1, [('environment_coverage', _p(environment_shift, shift=-1.5))]),
    'protein_hbond': ('trpcage20_7A', 1, [('protein_hbond', _p(protein_hbond_table))]),
    'nonlinear_coupling_environment': ('trpcage20_7A', 1, [('nonlinear_coupling_environment', _p(scaled, amp=0.3))]),
    'placement_fixed_point_vector_only': ('trpcage20_7A', 1, [('placement_fixed_point_vector_only', _p(noisy, amp=0.1))]),
    'placement_fixed_point_vector_only_CB': ('trpcage20_7A', 1, [('placement_fixed_point_vector_only_CB', _p(noisy, amp=0.3))]),
    'placement_fixed_point_vector_scalar': ('trpcage20_7A', 1, [('placement_fixed_point_vector_scalar', _p(noisy, amp=0.2))]),
    'hbond_sc_radial': ('proteinG56_restraints', 2, [('hbond_sc_radial', _p(radial_table))]),
    'placement_fixed_point_only_CB': ('proteinG56_restraints', 2, [('placement_fixed_point_only_CB', _p(noisy, amp=0.3))]),
    # The couplings to the environment carry under 3 % of this fixture's force (its springs dominate): with factors of at most
    # 1.3 no one of them moves the forces by 1e-2, so the two linear couplings travel with the spline coefficients, at a seed for
    # which the three together do.  Every node's own potential is still held to move (test_set_param_cases.py).
    'environment_couplings': ('proteinG56_restraints', 3, [('linear_coupling_uniform_env', _p(scaled, amp=0.3)),
                                                           ('linear_coupling_with_inactivation_env', _p(scaled, amp=0.3)),
                                                           ('nonlinear_coupling_environment', _p(scaled, amp=0.3))]),
    'environment_coverage_shrink_restraints': ('proteinG56_restraints', 2, [('environment_coverage', _p(environment_shift, shift=-1.5))]),
}
ALL_CASES = [c for c in CASES if c.startswith('all_')]
NODE_CASES = [c for c in CASES if not c.startswith(('all_', 'every_', 'md_'))]


def fixture_of(case):
    return CASES[case][0]


def nodes_of(case):
    return [n for n, _ in CASES[case][2]]


def extras(fixture):
    """the extra coordinate and potential nodes evaluate_all reads on this fixture"""
    return (P.RESTRAINT_COORDS, P.RESTRAINT_POTENTIALS) if fixture == 'proteinG56_restraints' else ((), ())


def potential_names(fixture):
    return P.POTENTIAL_NODES + list(extras(fixture)[1])


def own_key(fixture, node):
    """the key of the node's own result in evaluate_all: its potential, or its output"""
    return ('pot/' if node in potential_names(fixture) else 'out/') + node


def positions(fixture):
    """(pos, pos2): the golden structure and a second one within the margin of the cached pair lists"""
    g = P.golden(fixture)
    if 'pos2' in g:
        return g['pos'], g['pos2']
    return g['pos'], g['pos'] + np.float32(0.05) * np.random.RandomState(3).normal(size=g['pos'].shape).astype('f4')


def table_shape(path, node):
    grp, ds = TABLES[node]
    with P.pkg.h5lite.open_file(path, 'r') as t:
        g = t.group('input/potential/' + grp)
        shape = tuple(g.shape(ds))
        del g
    return shape


def read_table(path, node):
    """the node's table as set_param takes it and get_param gives it: f4, flat, file order"""
    grp, ds = TABLES[node]
    with P.pkg.h5lite.open_file(path, 'r') as t:
        g = t.group('input/potential/' + grp)
        v = np.asarray(g.read(ds)).astype('f4').ravel()
        del g
    return v


def build(case, dst):
    """copy of the case's fixture at dst with the perturbed tables; returns (old, new): dicts node -> flat f4 table"""
    fixture, seed, plan = CASES[case]
    H.copy_fixture(fixture, dst)
    rs = np.random.RandomState(seed)
    old = {}
    for node, (fn, kw) in plan:
        grp, ds = TABLES[node]
        old[node] = read_table(P.fixture(fixture), node)
        H.rewrite_in_place(str(dst), grp, ds, lambda T: fn(T, rs, **kw))
        gc.collect()      # (every h5lite handle is released before the file is opened again)
    new = dict((node, read_table(str(dst), node)) for node, _ in plan)
    return old, new
