"""Worker of test_gpu_accumulator_range.py::test_every_form_of_the_passes: evaluates one configuration at the given structures through
the product library under whatever UPSIDE_HIP_* environment the parent set (the switches are read once per process) and saves every
node's output and sensitivity, the potentials, the energy and the forces."""
import sys
import numpy as np
import parity_util as P

config, structures, out = sys.argv[1:4]
pos = np.load(structures)
up = P.pkg.Upside(config)
res = {}
for tag in pos.files:
    for k, v in P.evaluate_all(up, pos[tag]).items():
        res[tag + ':' + k] = v
up.close()
np.savez(out, **res)
