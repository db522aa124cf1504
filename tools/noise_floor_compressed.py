#!/usr/bin/env python3
"""Noise floor of the REFERENCE on the compressed structures and on the chain D cases (steeper hbond_coverage tables, which the
side-chain solve sees) of tests/accumulator_cases.py (build container only), by the method of
tools/noise_floor.py: the reference built -O1 without fast-math (tools/build_ref_O1.sh) against its -O3 -ffast-math build
(oracle/_ref) on exactly the coordinates and files the test uses.  Adds one entry per case (AC.noise_floor_key, AC.chain_key) to
tests/golden/reference_noise_floor.json and leaves the others as they are."""
import sys, os, json
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import parity_util as P, accumulator_cases as AC, numpy as np
O1 = P.pkg.UpsideLibrary('/tmp/refO1_7A/libupside_O1.so')
O3 = P.reference_library('7A')
orc = P.oracle_library()
path = os.path.join(ROOT, 'tests', 'golden', 'reference_noise_floor.json')
table = json.load(open(path))
import tempfile
tmp = tempfile.mkdtemp()
cases = [(AC.noise_floor_key(name, factor), P.fixture(name), AC.compressed_positions(name, factor)) for name, factor in AC.COMPRESSED]
cases += [(AC.chain_key(name, which, chain, k), AC.write_case(tmp, name, chain, k), AC.positions(name, which))
          for name, which in AC.STRUCTURES for chain, k in AC.RANGE_CASES if chain == 'D' and k > 1.]
for key, config, x in cases:
    res = {}
    for tag, lib in (('O1', O1), ('O3', O3), ('oracle', orc)):
        up = P.pkg.Upside(config, library=lib)
        res[tag] = P.evaluate_all(up, x)
    g = res['O3']
    sens = [k for k in g if k.startswith('sens/') and np.asarray(g[k]).size]
    entry = dict(deriv=float(P.rel_rms(g['deriv'], res['O1']['deriv'])), oracle_deriv=float(P.rel_rms(g['deriv'], res['oracle']['deriv'])),
                 sens=max(float(P.rel_rms(g[k], res['O1'][k])) for k in sens), oracle_sens=max(float(P.rel_rms(g[k], res['oracle'][k])) for k in sens))
    table[key] = {'pos': entry}
    print(key, entry)
json.dump(table, open(path, 'w'), indent=1, sort_keys=True)
