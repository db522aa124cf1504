"""Cases of test_gpu_accumulator_range.py: force fields 2^-16 .. 2^16 times as steep as the shipped one, and compressed structures.

The pair passes sum the partner side of every pair gradient in 64-bit fixed point (pair2_device.h: 2^-22 counts in the packed passes,
device_math.h: 2^-32 counts in the scalar ones).  With the shipped force field a contribution stays below ~50 even on a structure
compressed to 0.7 of its size, an order of magnitude under the 512 at which the packed passes' 32-bit conversion ends, so range is
reached through the force field: the environment coupling (chain A: exactly linear in its coefficients, and the side-chain solve
does not see it), the hydrogen-bond energy (chain B) or both (chain C), scaled by powers of two, which are exact in fp32.
None of the three reaches the PACKED passes, though: those serve the hbond_coverage graphs and the side-chain gradient, whose pair
sensitivities are rotamer marginals (at most 1) whatever the force field; the environment graph runs the scalar passes.  Chain D
therefore scales the radial pieces of the two hbond_coverage tables, which makes every pair gradient of the packed coverage pass
exactly k times as large (a bead's total is 16 at k = 1 and 4e3 at 2^8, where single contributions pass 512; 1e6 at 2^16).  The
side-chain solve sees these energies; the oracle's still converges in 8 to 12 iterations at every factor.
rotamer/pair_interaction/interaction_param is NOT scaled: the table holds more than energies (the oracle returns NaN from a factor
8 on); the side-chain gradient pass shares the conversion helper with the coverage passes and sees the compressed structures."""
import numpy as np
import parity_util as P
import hamiltonian_files as H

K_VALUES = [2. ** -16, 2. ** -8, 1., 2. ** 4, 2. ** 8, 2. ** 12, 2. ** 16]
K_RANGE = [k for k in K_VALUES if k >= 1.]
K_SMALL = [k for k in K_VALUES if k < 1.]
CHAINS = ['A', 'B', 'C', 'D']
# Chain D is there for range, so it starts where single contributions pass 512.  At 2^4 nothing is near the limit, but the side-chain
# solve sits between its two regimes there and the convergence threshold of the solve, amplified by the steeper table, shows in
# the forces: 1.4e-5 against the oracle on trpcage20_7A (marginals 3e-6 apart, both solves converged), with and without the wide path.
RANGE_CASES = [(chain, k) for chain in CHAINS for k in K_RANGE if not (chain == 'D' and 1. < k < 2. ** 8)]
N_RADIAL_7A = 24          # 2 n_knot coefficients of the two radial pieces in the 7 A tables (both fixtures used here)
STRUCTURES = [('trpcage20_7A', 'initial_pos'), ('proteinG56_7A', 'initial_pos'), ('proteinG56_7A', 'pos2')]
# chain A: the coupling's sensitivity and the two sides of the environment_coverage pair graph it flows back through
CHAIN_A_SENS = ['sens/environment_coverage', 'sens/weighted_pos', 'sens/placement_fixed_point_vector_only_CB']

# compressed structures at force-field scale (coordinates scaled about the centroid); the oracle's side-chain solve converges on all of
# them (syn300_10A at 0.7, where it runs to its 1000-iteration cap, is left out)
COMPRESSED = [('trpcage20_7A', 0.8), ('trpcage20_7A', 0.7), ('proteinG56_7A', 0.8)]
ROTAMER_ITERATION_CAP = 1000


def klabel(k):
    return '2^%d' % int(round(np.log2(k)))


def positions(name, which):
    if which == 'initial_pos':
        with P.pkg.h5lite.open_file(P.fixture(name)) as t:
            return t.read('input/pos', 'f4')[:, :, 0].copy()
    return P.golden(name)[which].astype('f4')


def compressed_positions(name, factor):
    x = positions(name, 'initial_pos').astype('f8')
    c = x.mean(axis=0)
    return (c + factor * (x - c)).astype('f4')


def noise_floor_key(name, factor):
    """entry of tests/golden/reference_noise_floor.json for a compressed structure"""
    return '%s@%.1f' % (name, factor)


def chain_key(name, which, chain, k):
    """entry of tests/golden/reference_noise_floor.json for a case of a chain the side-chain solve sees"""
    return '%s/%s/%s/%s' % (name, which, chain, klabel(k))


def write_case(directory, name, chain, k):
    """a copy of the fixture with chain `chain` scaled by k; returns its path"""
    path = H.copy_fixture(name, '%s/%s_%s_%s.up' % (directory, name, chain, klabel(k)))
    if chain in ('A', 'C'):
        H.scale_coupling(path, k)
    if chain in ('B', 'C'):
        H.scale_hbond(path, k)
    if chain == 'D':
        H.scale_coverage(path, k, N_RADIAL_7A)
    return path


def longest_row(edges):
    """the largest number of pairs any one element of either side of a pair list takes part in"""
    e = np.asarray(edges)
    if not len(e):
        return 0
    return int(max(np.bincount(e[:, 0]).max(), np.bincount(e[:, 1]).max()))
