"""Worker of tests/test_gpu_rotamer_multibead.py: the several-beads-per-state configuration through the product library under whatever
UPSIDE_HIP_* environment the parent set (the switches are read once per process).  A one-system engine with every node's output and the
side-chain node's named values; a 3-system engine (pos, pos2, pos) with energies, forces, each system's parameter derivative and pair
list, the forms its solve ran in, ten repeated evaluations, and 4 MD rounds (12 steps) from the first structure."""
import ctypes as ct
import hashlib
import sys
import numpy as np
import parity_util as P
import rotamer_multibead as M
import rotamer_forms_cases as C

path, out, posfile, n_type = sys.argv[1], sys.argv[2], sys.argv[3], int(sys.argv[4])
pos = np.load(posfile)['pos'].astype('f4')
res = {}
up = P.pkg.Upside(path)
for k, v in M.record(up, path, n_type).items():
    res['one/' + k] = v
n = int(res['one/rotamer/n_node'])
res['one/rotamer/edge_energy'] = up.get_value_by_name((n, n, 6, 6), 'rotamer', 'edge_energy')
res['one/n_bad'] = up.get_value_by_name((1,), 'rotamer', 'read n_bad_solve')
for k, v in C.read_form(up.calc, up.engine, 1).items():
    res['one_form/' + k] = np.asarray(v)
up.close()

S = pos.shape[0]
ens = P.pkg.engine.Ensemble(path, S)
c = ens.calc
c.upside_hip_get_param_deriv.argtypes = [ct.c_void_p, ct.c_char_p, ct.c_int, ct.c_int, ct.c_void_p]
c.upside_hip_get_pairlist.restype = ct.c_int
c.upside_hip_get_pairlist.argtypes = [ct.c_void_p, ct.c_char_p, ct.c_int, ct.c_int, ct.c_void_p, ct.c_void_p]
ens.set_pos(pos)
e, d = ens.energies_and_derivs()
res['ens_energy'] = e; res['ens_force'] = d
pd = np.zeros((S, n_type, n_type, 62), 'f4')
for s in range(S):
    assert c.upside_hip_get_param_deriv(ens.engine, b'rotamer', s, pd[s].size, pd[s].ctypes.data) == 0
    i1 = np.zeros(400000, 'i4'); i2 = np.zeros(400000, 'i4')
    m = c.upside_hip_get_pairlist(ens.engine, b'rotamer', s, i1.size, i1.ctypes.data, i2.ctypes.data)
    assert 0 <= m <= i1.size
    res['ens_pairs%d' % s] = np.column_stack((i1[:m], i2[:m]))
res['ens_param_deriv'] = pd
for k, v in C.read_form(c, ens.engine, S).items():
    res['ens_form/' + k] = np.asarray(v)
seen = set(); worst = 0.
for k in range(10):
    e2, d2 = ens.energies_and_derivs()
    seen.add(hashlib.sha256(e2.tobytes() + d2.tobytes()).hexdigest())
    worst = max(worst, P.rel_rms(d, d2))
res['repeat_distinct'] = np.int32(len(seen | {hashlib.sha256(e.tobytes() + d.tobytes()).hexdigest()}))
res['repeat_worst'] = np.float64(worst)
ens.set_pos(np.stack([pos[0]] * S))
ens.init_md(0.8, 12345, 5.0, 0.009, 1)
ens.run_rounds(4)
res['md_pos'] = ens.get_pos(); res['md_mom'] = ens.get_mom()
ens.close()
np.savez(out, **res)
