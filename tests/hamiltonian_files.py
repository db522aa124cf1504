"""Configuration files of Hamiltonian ladders for the tests: copies of a fixture with some /input/potential values changed
(written with h5lite; datasets keep their type, shape and attributes)."""
import shutil
import numpy as np
import parity_util as P


def rewrite(path, node, name, fn):
    """dataset `name` of node `node` := fn(old values), same dtype; its attributes are kept"""
    with P.pkg.h5lite.open_file(path, 'r+') as t:
        g = t.group('input/potential/' + node)
        old = np.asarray(g.read(name))
        attrs = {a: g.get_attr(a, name) for a in ('time_initial', 'time_step') if g.has_attr(a, name)}
        new = np.asarray(fn(old.copy()))
        g.delete(name)
        g.write(name, new.astype(old.dtype))
        for a, v in attrs.items():
            g.set_attr(a, v, obj=name)


def scale_hbond(path, factor):
    with P.pkg.h5lite.open_file(path, 'r+') as t:
        g = t.group('input/potential/hbond_energy')
        g.set_attr('protein_hbond_energy', np.float64(factor * float(np.asarray(g.get_attr('protein_hbond_energy')).ravel()[0])))


def rewrite_in_place(path, node, name, fn):
    """dataset `name` of node `node` := fn(old values), written IN PLACE: type, shape and every attribute of the dataset stay what
    they were (rewrite() re-creates the dataset and carries only time_* over, which loses e.g. coeff's spline_offset / spline_inv_dx)"""
    h5 = P.pkg.h5lite
    with h5.open_file(path, 'r+') as t:
        g = t.group('input/potential/' + node)
        old = np.asarray(g.read(name))
        new = np.ascontiguousarray(np.asarray(fn(old.copy())).astype(old.dtype))
        assert new.shape == old.shape
        L = h5.lib()
        d = L.H5Dopen2(g.hid, name.encode(), 0)
        if d < 0:
            raise IOError('cannot open %s/%s of %s' % (node, name, path))
        try:
            if L.H5Dwrite(d, h5._native(new.dtype), 0, 0, 0, new.ctypes.data) < 0:
                raise IOError('cannot write %s/%s of %s' % (node, name, path))
        finally:
            L.H5Dclose(d)
        del g


def scale_dataset(path, node, name, k):
    """dataset `name` of node `node` *= k; every attribute of the dataset is kept"""
    rewrite_in_place(path, node, name, lambda v: v * k)


def scale_coupling(path, k):
    """the environment coupling's energy scale (every spline coefficient of nonlinear_coupling_environment)"""
    scale_dataset(path, 'nonlinear_coupling_environment', 'coeff', k)


def scale_coverage(path, k, n_radial):
    """the energy scale of the side-chain / backbone hydrogen-bond coverage: the two radial pieces (the last n_radial = 2 n_knot
    coefficients of every row of interaction_param) of both coverage graphs times k.  The angular pieces in front of them are weights,
    not energies, and stay; a pair's value and its whole gradient are then exactly k times what they were."""
    def radial(v):
        v[..., -n_radial:] *= k
        return v
    for node in ('hbond_coverage', 'hbond_coverage_hydrophobe'):
        rewrite_in_place(path, node, 'interaction_param', radial)


def copy_fixture(name, dst):
    shutil.copyfile(P.fixture(name), str(dst))
    return str(dst)


def vary_table(path, i):
    """window i of a ladder that varies every row of the per-system table of proteinG56_restraints at once"""
    f = 1. + 0.05 * i
    rewrite(path, 'dist_spring', 'equil_dist', lambda v: v * (1. + 0.01 * i))
    rewrite(path, 'dist_spring', 'spring_const', lambda v: v * f)
    rewrite(path, 'angle_spring', 'spring_const', lambda v: v * f)
    rewrite(path, 'dihedral_spring', 'equil_dist', lambda v: v + 0.02 * i)
    rewrite(path, 'atom_pos_spring', 'x0', lambda v: v + 0.3 * i)
    rewrite(path, 'atom_pos_spring', 'spring_const', lambda v: v * f)
    rewrite(path, 'tension', 'tension_coeff', lambda v: v * f)
    rewrite(path, 'AFM', 'spring_const', lambda v: v * f)
    rewrite(path, 'AFM', 'starting_tip_pos', lambda v: v + 0.5 * i)
    rewrite(path, 'AFM', 'pulling_vel', lambda v: v * f)
    rewrite(path, 'z_flat_bottom', 'z0', lambda v: v + 0.2 * i)
    rewrite(path, 'z_flat_bottom', 'radius', lambda v: v * f)
    rewrite(path, 'contact', 'energy', lambda v: v * f)
    rewrite(path, 'contact', 'distance', lambda v: v + 0.1 * i)
    rewrite(path, 'contact', 'width', lambda v: v * f)
    scale_hbond(path, 1. - 0.02 * i)
