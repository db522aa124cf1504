"""Worker of tests/test_gpu_rotamer_forms.py: evaluates the systems of a position file through the product library under whatever
UPSIDE_HIP_* environment the parent set (the switches are read once per process), and saves energies, forces and the side-chain node's
report of the forms its solve ran in.  Up to 3 systems it also evaluates the first two through a one-system engine, the first with every
node's output."""
import sys
import numpy as np
import parity_util as P
import rotamer_forms_cases as C

name, out, posfile = sys.argv[1:4]
pos = np.load(posfile)['pos'].astype('f4')
S = pos.shape[0]
res = {}


def save_form(prefix, form):
    for k, v in form.items():
        res[prefix + k] = np.asarray(v)


if S <= 3:
    up = P.pkg.Upside(P.fixture(name))
    for k, v in P.evaluate_all(up, pos[0]).items():
        res['one/' + k] = v
    res['one_energy2'] = np.float32(up.energy(pos[1])); res['one_force2'] = up.deriv(pos[1])
    save_form('one_form/', C.read_form(up.calc, up.engine, 1))
    up.close()
ens = P.pkg.engine.Ensemble(P.fixture(name), S)
ens.set_pos(pos)
e, d = ens.energies_and_derivs()
res['ens_energy'] = e; res['ens_force'] = d
save_form('ens_form/', C.read_form(ens.calc, ens.engine, S))
ens.close()
np.savez(out, **res)
