"""CPU tests of the TorusDBN backbone prior's configuration writer (config.add_torus_dbn) and of the float64 yardstick the GPU
tests compare against (tests/hmm_reference.py): the yardstick is pinned against explicit enumeration of the state paths and
against central differences of its own -log Z before anything is measured with it."""
import ctypes as ct
import os
import shutil
import numpy as np
import pytest
import parity_util as P
import hmm_reference as R

cfg = P.pkg.config
h5lite = P.pkg.h5lite


# ---- the yardstick -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_state,n_residue', [(3, 4), (2, 1)])
def test_yardstick_matches_explicit_enumeration(n_state, n_residue):
    rs = np.random.RandomState(10 * n_state + n_residue)
    e = rs.normal(size=(n_residue, n_state)) * 2.
    E = rs.uniform(0., 3., size=(n_state, n_state))
    pot, marg, counts = R.brute_force(e, E)
    fb = R.forward_backward(e, E)
    assert abs(R.neg_log_z(e, E) - pot) <= 1e-12 and abs(fb['pot'] - pot) <= 1e-12
    assert np.abs(fb['marginals'] - marg).max() <= 1e-12 and np.abs(fb['sens'] - marg).max() <= 1e-12
    assert np.abs(fb['counts'] - counts).max() <= 1e-12
    assert np.abs(marg.sum(axis=1) - 1.).max() <= 1e-12 and abs(counts.sum() - (n_residue - 1)) <= 1e-12
    if n_residue == 1:      # one residue: no transition, -log Z = -log sum_s exp(-e[0, s])
        assert not counts.any() and abs(pot + np.log(np.exp(-e[0]).sum())) <= 1e-12


def test_yardstick_index_selects_and_orders_the_chain():
    rs = np.random.RandomState(5)
    e = rs.normal(size=(6, 3)); E = rs.uniform(0., 2., size=(3, 3))
    index = np.array([4, 2, 0, 5])
    fb = R.forward_backward(e, E, index)
    direct = R.forward_backward(e[index], E)
    assert abs(fb['pot'] - direct['pot']) <= 1e-14 and abs(R.neg_log_z(e, E, index) - direct['pot']) <= 1e-14
    assert np.array_equal(fb['sens'][index], direct['marginals']) and not fb['sens'][[1, 3]].any()
    assert not np.allclose(R.forward_backward(e, E, index[::-1])['pot'], fb['pot'])      # T is not symmetric: the direction matters


def _central(f, x, h):
    d = np.zeros_like(x)
    it = np.nditer(x, flags=['multi_index'])
    for _ in it:
        i = it.multi_index
        x0 = x[i]
        x[i] = x0 + h; fp = f()
        x[i] = x0 - h; fm = f()
        x[i] = x0
        d[i] = (fp - fm) / (2. * h)
    return d


def test_yardstick_derivatives_match_central_differences_of_its_minus_log_z():
    """step 1e-6; every element within 1e-7 of the difference quotient, relative to the largest element (derivatives of order one)"""
    h = 1e-6
    rs = np.random.RandomState(8)
    n_rama, n_state, n_restype = 11, 5, 4
    par = {k: np.asarray(v, 'f8') if k != 'restype_order' else v for k, v in R.random_parameters(n_state, 3).items()}
    par['aa_basin_energy'] = par['aa_basin_energy'][:n_restype].copy()
    par['id'] = np.arange(1, n_rama - 1); par['restypes'] = rs.randint(0, n_restype, size=n_rama - 2)
    rama = rs.uniform(-np.pi, np.pi, size=(n_rama, 2))
    back = R.prior_backward(rama, par)
    energy = lambda: R.prior_energy(rama, par)
    assert abs(back['pot'] - energy()) <= 1e-13

    def close(analytic, numeric, what):
        scale = np.abs(numeric).max()
        assert 0.05 < scale < 20., (what, scale)
        err = np.abs(np.asarray(analytic) - numeric).max() / scale
        print('%-24s largest deviation / scale %.2e' % (what, err))
        assert err <= 1e-7, (what, err)

    fd = _central(energy, rama, h)
    close(back['d_rama'], fd, 'phi / psi')
    assert not fd[0].any() and not fd[-1].any()
    close(back['d_prior'], _central(energy, par['aa_basin_energy'], h), 'prior_offset_energies')
    close(back['counts'], _central(energy, par['transition_energy'], h), 'transition_energy')
    e = back['energy'].copy()
    close(back['sens'], _central(lambda: R.neg_log_z(e, par['transition_energy']), e, h), 'emission energies')
    # a reversed chain: the gradient lands at index[r]
    rev = par['id'].shape[0] - 1 - np.arange(par['id'].shape[0])
    fb = R.forward_backward(e, par['transition_energy'], rev)
    close(fb['sens'], _central(lambda: R.neg_log_z(e, par['transition_energy'], rev), e, h), 'reversed chain')


def test_yardstick_is_finite_on_energies_spanning_sixty():
    rs = np.random.RandomState(2)
    n, ns = 18, 7
    e = rs.uniform(0., 60., size=(n, ns)); e[:, 0] = 0.; e[::2, -1] = 60.
    E = rs.uniform(0., 60., size=(ns, ns)); E[0, 0] = 0.; E[1, 2] = 60.
    fb = R.forward_backward(e, E)
    assert np.isfinite(fb['pot']) and np.isfinite(fb['marginals']).all() and np.isfinite(fb['counts']).all()
    assert np.abs(fb['marginals'].sum(axis=1) - 1.).max() <= 1e-12 and abs(fb['counts'].sum() - (n - 1)) <= 1e-11
    assert np.isfinite(R.energy_offset(E)) and 0. <= R.energy_offset(E) <= 60.


def test_emission_matrix_follows_the_sign_convention():
    bp = np.array([[0.5, 2., 0.3, 3., -1.1, 0.7]])
    M = R.cs_to_emission(bp)[:, 0]
    assert np.allclose(M, [-2. * np.cos(0.3), -2. * np.sin(0.3), -3. * np.cos(-1.1), -3. * np.sin(-1.1), 0.7 * np.cos(1.4), 0.7 * np.sin(1.4)])
    rama = np.array([[0.3, -1.1]])      # at the basin's centre: -kappa_phi - kappa_psi + kappa_cor + log norm + prior
    e = R.emission_energies(rama, [0], [0], np.array([[0.25]]), bp)
    assert abs(e[0, 0] - (0.25 + 0.5 - 2. - 3. + 0.7)) <= 1e-14


# ---- config.add_torus_dbn ----------------------------------------------------------------------------------------------------
def test_add_torus_dbn_writes_the_schema(tmp_path):
    path = str(tmp_path / 'dbn.up')
    par = R.append_hmm(P.fixture('trpcage20_7A'), path, n_state=7, seed=4)
    assert par['names'] == ['torus_dbn', 'fixed_hmm']
    with h5lite.open_file(path) as f:
        pot = f.group('input/potential')
        seq = [x.decode() for x in f.read('input/sequence')]
        n_res = len(seq)
        assert n_res == 20
        g = pot.group('torus_dbn')
        assert list(g.get_attr('arguments')) == ['rama_coord']
        ids = g.read('id'); rt = g.read('restypes')
        assert ids.dtype.kind == 'i' and rt.dtype.kind == 'i'
        assert np.array_equal(ids, np.arange(1, n_res - 1))
        assert [R.RESTYPE_ORDER[t] for t in rt] == seq[1:-1]
        fp = g.read('prior_offset_energies'); fb = g.read('basin_param')
        assert fp.dtype == np.float32 and fb.dtype == np.float32
        assert fp.shape == (len(R.RESTYPE_ORDER), 7) and np.array_equal(fp, par['aa_basin_energy'])
        assert fb.shape == (7, 6) and np.array_equal(fb, par['basin_param'])
        g = pot.group('fixed_hmm')
        assert list(g.get_attr('arguments')) == ['torus_dbn']
        assert np.array_equal(g.read('index'), np.arange(n_res - 2)) and g.read('index').dtype.kind == 'i'
        ft = g.read('transition_energy')
        assert ft.dtype == np.float32 and ft.shape == (7, 7) and np.array_equal(ft, par['transition_energy'])
        del g, pot      # (an open group keeps the file open)
    named = cfg.add_torus_dbn(path, par['basin_param'], par['aa_basin_energy'], par['transition_energy'], par['restype_order'], name='second')
    assert named == ['torus_dbn_second', 'fixed_hmm_second']
    with h5lite.open_file(path) as f:
        assert list(f.group('input/potential/fixed_hmm_second').get_attr('arguments')) == ['torus_dbn_second']
    with pytest.raises(ValueError, match='already has a node'):
        cfg.add_torus_dbn(path, par['basin_param'], par['aa_basin_energy'], par['transition_energy'], par['restype_order'])


def test_add_torus_dbn_refuses_bad_input(tmp_path):
    path = str(tmp_path / 'dbn.up')
    shutil.copyfile(P.fixture('trpcage20_7A'), path)
    os.chmod(path, 0o644)
    p = R.random_parameters(5, 1)
    bp, aa, te, order = p['basin_param'], p['aa_basin_energy'], p['transition_energy'], p['restype_order']
    with pytest.raises(ValueError, match='basin_param'):
        cfg.add_torus_dbn(path, bp[:, :5], aa, te, order)
    with pytest.raises(ValueError, match='aa_basin_energy'):
        cfg.add_torus_dbn(path, bp, aa[:, :4], te, order)
    with pytest.raises(ValueError, match='transition_energy'):
        cfg.add_torus_dbn(path, bp, aa, te[:, :4], order)
    with pytest.raises(ValueError, match='restype_order'):
        cfg.add_torus_dbn(path, bp, aa, te, order[:-1])
    with h5lite.open_file(path) as f:
        seq = [x.decode() for x in f.read('input/sequence')]
    gone = seq[5]
    renamed = ['XXX' if x == gone else x for x in order]
    with pytest.raises(ValueError, match='residue name %s is not in restype_order' % gone):
        cfg.add_torus_dbn(path, bp, aa, te, renamed)
    with h5lite.open_file(path, 'r+') as f:      # the refused calls wrote nothing
        pot = f.group('input/potential')
        assert not [k for k in pot.keys() if k.startswith(('torus_dbn', 'fixed_hmm'))]
        pot.delete('rama_coord')
    with pytest.raises(ValueError, match='no rama_coord node'):
        cfg.add_torus_dbn(path, bp, aa, te, order)
    short = str(tmp_path / 'short.up')
    shutil.copyfile(P.fixture('trpcage20_7A'), short)
    os.chmod(short, 0o644)
    with h5lite.open_file(short, 'r+') as f:
        inp = f.group('input')
        two = inp.read('sequence')[:2]
        inp.delete('sequence'); inp.write('sequence', two)
    with pytest.raises(ValueError, match='at least 3'):
        cfg.add_torus_dbn(short, bp, aa, te, order)


# ---- the library -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(P.pkg.PRODUCT_LIB):
        pytest.fail('libupside_hip.so not built (run __graft_entry__.build())')
    return ct.CDLL(P.pkg.PRODUCT_LIB)


def test_node_types_are_registered(lib):
    lib.upside_hip_node_type_registered.argtypes = [ct.c_char_p]
    assert lib.upside_hip_node_type_registered(b'torus_dbn') == 1
    assert lib.upside_hip_node_type_registered(b'fixed_hmm') == 1


def test_launchers_are_declared_and_exported(lib):
    kernels_h = open(os.path.join(P.ROOT, 'include', 'upside_hip_kernels.h')).read()
    for n in ('upk_torus_dbn_fwd', 'upk_torus_dbn_bwd', 'upk_torus_dbn_param_deriv', 'upk_torus_dbn_param_deriv_all', 'upk_fixed_hmm',
              'upk_fixed_hmm_max_state', 'upk_fixed_hmm_param_deriv', 'upk_fixed_hmm_param_deriv_all'):
        assert n + '(' in kernels_h and hasattr(lib, n), n
    lib.upk_fixed_hmm_max_state.restype = ct.c_int
    assert lib.upk_fixed_hmm_max_state() == 128
