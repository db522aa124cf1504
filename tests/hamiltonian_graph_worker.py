"""Worker of test_hamiltonian_batch.py::test_ladder_md_under_graph_capture: MD of an hbond_energy ladder under whatever
UPSIDE_HIP_GRAPH the parent set (read once per process), with a per-system set_param between two run_steps calls."""
import sys
import numpy as np
import parity_util as P

out, files = sys.argv[1], sys.argv[2:]
ens = P.pkg.engine.Ensemble.from_files(files)
ens.set_pos(P.golden('proteinG56_7A')['pos'])
ens.init_md(np.linspace(0.8, 0.9, len(files)), 5)
ens.run_steps(30)
mid = ens.get_pos()
ens.set_param([0.7 * float(ens.get_param((1,), 'hbond_energy', system=1)[0])], 'hbond_energy', system=1)
ens.run_steps(30)
np.savez(out, mid=mid, pos=ens.get_pos(), mom=ens.get_mom(), energy=ens.energies())
ens.close()
