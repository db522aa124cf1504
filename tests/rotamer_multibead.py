"""A side-chain library with several beads per rotamer state, made from tests/golden/parameters/ff_1/sidechain.h5, and the protein G
configuration written with it (CPU only; used by tests/test_rotamer_multibead.py, tests/test_gpu_rotamer_multibead.py and
tools/make_fixtures.py --multibead).

Every shipped library has one bead per state, so each entry of a side-chain pair matrix has one contributing bead pair.  Here the
residue types of TWO_BEADS -- a 1-state, two 3-state and a 6-state type, 28 of protein G's 56 residues -- get a second bead per state:
1 A along the state's stored direction, with a bead type of its own whose rows and columns in the pair, coverage and hydrophobe tables
are the first bead's scaled by 0.5, and whose 1-body probability row is a copy.  Both beads contribute, so a dropped or double-counted
bead changes energies and forces at first order."""
import os
import numpy as np
import parity_util as P

NAME = 'multibead_proteinG56'
TWO_BEADS = ('ALA', 'THR', 'LYS', 'GLU')
PARAM = os.path.join(P.GOLDEN_DIR, 'parameters')
GOLDEN = os.path.join(P.GOLDEN_DIR, NAME + '.golden.npz')


def write_library(path, two_beads=TWO_BEADS, shift=1.0, scale=0.5):
    """the synthetic library; returns the number of bead types"""
    h5 = P.pkg.h5lite
    with h5.open_file(os.path.join(PARAM, 'ff_1', 'sidechain.h5')) as src:
        d = dict((nm, src.read(nm)) for nm in src.keys())
    restype = [x.decode() for x in d['restype_order']]
    beads = [x.decode() for x in d['bead_order']]
    n_old = len(beads)
    first = {}                                  # new bead type -> the type it copies
    centers, probs, start_stop = [], [], []
    for i, aa in enumerate(restype):
        start, stop, n_bead = [int(x) for x in d['rotamer_start_stop_bead'][i]]
        assert n_bead == 1
        new_start = len(centers)
        for row in range(start, stop):
            c = d['rotamer_center_fixed'][row].astype('f8')
            centers.append(c); probs.append(d['rotamer_prob'][:, :, row])
            if aa in two_beads:
                c2 = c.copy(); c2[:3] += shift * c[3:6] / max(np.sqrt((c[3:6] ** 2).sum()), 1e-12)
                centers.append(c2); probs.append(d['rotamer_prob'][:, :, row])
        if aa in two_beads:
            first[len(beads)] = beads.index(aa + '_0'); beads.append(aa + '_1')
        start_stop.append((new_start, len(centers), 2 if aa in two_beads else 1))
    n_type = len(beads)
    src_of = np.array([first.get(t, t) for t in range(n_type)])
    fac = np.where(np.arange(n_type) >= n_old, scale, 1.)
    pair = d['pair_interaction'].astype('f8')[src_of][:, src_of] * (fac[:, None] * fac[None, :])[:, :, None]
    cov = d['coverage_interaction'].astype('f8')[:, src_of] * fac[None, :, None]
    hyd = d['hydrophobe_interaction'].astype('f8')[:, src_of] * fac[None, :, None]
    with h5.open_file(path, 'w') as out:
        out.write('restype_order', d['restype_order'])
        out.write('bead_order', np.array(beads))
        out.write('rotamer_center_fixed', np.array(centers))
        out.write('rotamer_prob', np.stack(probs, axis=2))
        out.write('rotamer_start_stop_bead', np.array(start_stop, dtype='i8'))
        out.write('restype_and_chi_and_state', d['restype_and_chi_and_state'])
        out.write('pair_interaction', pair)
        out.write('coverage_interaction', cov)
        out.write('hydrophobe_placement', d['hydrophobe_placement'])
        out.write('hydrophobe_interaction', hyd)
    return n_type


def write_configuration(directory):
    """protein G (sequence and coordinates of the fixture proteinG56_7A) with the synthetic library; returns (path, info of write_config,
    number of bead types)"""
    cfg = P.pkg.config
    lib = os.path.join(str(directory), 'sidechain_multibead.h5')
    n_type = write_library(lib)
    with open(os.path.join(PARAM, 'ff_1', 'hbond')) as f:
        hbond_energy = float(f.read())
    path = os.path.join(str(directory), NAME + '.up')
    pos = np.load(os.path.join(P.GOLDEN_DIR, 'proteinG56_7A.coords.npy')).astype('f8')
    info = cfg.write_config(path, cfg.fasta_from_one_letter(cfg.PROTEIN_G), pos, sidechain_lib=lib,
                            environment_lib=os.path.join(PARAM, 'ff_1', 'environment.h5'),
                            rama_ref=np.load(os.path.join(PARAM, 'rama_reference.npy')), hbond_energy=hbond_energy, rama_seed=12,
                            per_residue_rama=True)
    return path, info, n_type


def beads_per_state(path):
    """{(n_rot, node index, state): number of beads} of a configuration's side-chain node"""
    with P.pkg.h5lite.open_file(path) as t:
        ids = t.group('input/potential/rotamer').read('pair_interaction/id', 'i4').astype('u4')
    count = {}
    for i in ids:
        k = (int((i >> 4) & 15), int(i >> 8), int(i & 15))
        count[k] = count.get(k, 0) + 1
    return count


def record(up, path, n_type):
    """what the golden file holds of one library (the reference's, when recording), at the configuration's own structure"""
    x = up.initial_pos.copy()
    g = P.evaluate_all(up, x)
    g['pos'] = x
    n = int(up.get_value_by_name((1,), 'rotamer', 'n_node')[0])
    g['rotamer/n_node'] = np.int32(n)
    g['rotamer/node_energy'] = up.get_value_by_name((n, 6), 'rotamer', 'node_energy')
    g['rotamer/rotamer_free_energy'] = up.get_value_by_name((n,), 'rotamer', 'rotamer_free_energy')
    g['rotamer/rotamer_1body_energy'] = up.get_value_by_name((n, 3), 'rotamer', 'rotamer_1body_energy')
    g['rotamer/count_edges_by_type'] = up.get_value_by_name((n_type, n_type), 'rotamer', 'count_edges_by_type')
    up.deriv(x)
    g['param_deriv/rotamer'] = up.get_param_deriv((n_type, n_type, 62), 'rotamer')
    return g
