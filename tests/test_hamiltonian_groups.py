"""CPU checks of the grouping upside_main uses for a run of several configuration files (upside_hip_group_configurations):
files that differ only in the values of the per-system table share one engine; any other difference makes a group of its
own; UPSIDE_HIP_HAMILTONIAN_BATCH=0 groups by the whole /input/potential.  HDF5 only, no GPU."""
import json
import os
import subprocess
import sys
import numpy as np
import pytest
import parity_util as P
import hamiltonian_files as H

BASE = 'proteinG56_restraints'


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(P.pkg.PRODUCT_LIB):
        pytest.skip('libupside_hip.so not built (run __graft_entry__.build())')
    return P.pkg.UpsideLibrary(P.pkg.PRODUCT_LIB)


def groups(lib, paths):
    return list(P.pkg.engine.group_configurations(paths, library=lib))


def variant(tmp_path, tag, change=None, base=BASE):
    p = H.copy_fixture(base, tmp_path / ('%s.up' % tag))
    if change:
        change(p)
    return p


def test_value_changes_share_a_group(lib, tmp_path):
    fs = [variant(tmp_path, 'base'),
          variant(tmp_path, 'hb', lambda p: H.scale_hbond(p, 0.9)),
          variant(tmp_path, 'eq', lambda p: H.rewrite(p, 'dist_spring', 'equil_dist', lambda v: v * 1.02)),
          variant(tmp_path, 'tn', lambda p: H.rewrite(p, 'tension', 'tension_coeff', lambda v: v * 2.)),
          variant(tmp_path, 'ct', lambda p: H.rewrite(p, 'contact', 'energy', lambda v: v * 0.5)),
          variant(tmp_path, 'all', lambda p: H.vary_table(p, 3)),
          variant(tmp_path, 'base2')]
    assert groups(lib, fs) == [0] * len(fs)


@pytest.mark.parametrize('what', ['id', 'rama', 'shape', 'other_fixture', 'afm_clock'])
def test_structural_changes_make_groups(lib, tmp_path, what):
    change = {
        'id': lambda p: H.rewrite(p, 'dist_spring', 'id', lambda v: v[::-1].copy()),
        'rama': lambda p: H.rewrite(p, 'rama_map_pot', 'rama_pot', lambda v: v * 1.01),
        'shape': lambda p: H.rewrite(p, 'contact', 'energy', lambda v: np.concatenate([v, v[:1]])),
        'other_fixture': None,
        'afm_clock': lambda p: _set_afm_clock(p),
    }[what]
    other = variant(tmp_path, 'x', change, base='proteinG56_7A' if what == 'other_fixture' else BASE)
    base = variant(tmp_path, 'base')
    hb = variant(tmp_path, 'hb', lambda p: H.scale_hbond(p, 0.9))
    assert groups(lib, [base, other, hb]) == [0, 1, 0]


def _set_afm_clock(p):
    with P.pkg.h5lite.open_file(p, 'r+') as t:
        g = t.group('input/potential/AFM')
        g.set_attr('time_step', np.float32(2. * float(np.asarray(g.get_attr('time_step', 'pulling_vel')).ravel()[0]) + 1.), obj='pulling_vel')


def test_batch_off_groups_by_whole_potential(lib, tmp_path):
    fs = [variant(tmp_path, 'base'),
          variant(tmp_path, 'hb', lambda p: H.scale_hbond(p, 0.9)),
          variant(tmp_path, 'eq', lambda p: H.rewrite(p, 'dist_spring', 'equil_dist', lambda v: v * 1.02)),
          variant(tmp_path, 'base2'),
          variant(tmp_path, 'hb2', lambda p: H.scale_hbond(p, 0.9))]
    code = ('import sys, json; sys.path.insert(0, %r); sys.path.insert(0, %r); import parity_util as P; '
            'print(json.dumps([int(x) for x in P.pkg.engine.group_configurations(%r, library=P.pkg.UpsideLibrary(P.pkg.PRODUCT_LIB))]))'
            % (P.ROOT, os.path.join(P.ROOT, 'tests'), fs))
    out = subprocess.run([sys.executable, '-c', code], check=True, stdout=subprocess.PIPE, timeout=300,
                         env=dict(os.environ, UPSIDE_HIP_HAMILTONIAN_BATCH='0')).stdout.decode().strip().splitlines()[-1]
    assert json.loads(out) == [0, 1, 2, 0, 1]
    assert groups(lib, fs) == [0] * 5          # (and with the default: one ladder)


def test_header_and_bindings(lib):
    txt = open(os.path.join(P.ROOT, 'include', 'upside_engine_c.h')).read()
    for n in ('upside_hip_construct_files', 'upside_hip_group_configurations', 'upside_hip_set_param_system',
              'upside_hip_get_param_system', 'upside_hip_hamiltonian_swap'):
        assert n + '(' in txt, n
        assert hasattr(lib.calc, n), n
    for m in ('from_files', 'set_param', 'get_param', 'hamiltonian_swap'):
        assert callable(getattr(P.pkg.engine.Ensemble, m))
