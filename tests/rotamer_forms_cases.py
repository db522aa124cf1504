"""Cases of tests/test_gpu_rotamer_forms.py and the CPU-side check that a fixture can tell a wrong fold from a right one.

The side-chain solve keeps its pair matrices as exp(-E) (`p_prob`: every shipped library) or as E ("energy form": several beads per state,
UPSIDE_HIP_ROTAMER_ATOMIC=1, UPSIDE_HIP_BP_ENERGY_TABLE=1, every cluster solve).  What a LARGE batch selects -- the one-workgroup solve, node
probabilities by a kernel of their own, from 512 systems on the inbox layout and the fold of the 1-state partners as a launch in front of
the solve -- is forced here at 3 systems and crossed with the stand-ins of the energy form."""
import numpy as np
import parity_util as P

# the large-batch selection forced at small size
BASE = {'UPSIDE_HIP_BP_CLUSTER': '1', 'UPSIDE_HIP_BATCH': '0', 'UPSIDE_HIP_GRAPH': '0', 'UPSIDE_HIP_NODE_PROB_IN_SOLVE': '0'}

ATOMIC = {'UPSIDE_HIP_ROTAMER_ATOMIC': '1'}
TABLE = {'UPSIDE_HIP_BP_ENERGY_TABLE': '1'}


def _layout(v):
    return {'UPSIDE_HIP_BP_LAYOUT': str(v)}


# (tag, switches on top of BASE).  The control comes first.
CASES = [
    ('control', {}),
    ('layout1', _layout(1)),                                  # probability form through the pre-fold: what 512 systems run today
    ('atomic', dict(ATOMIC)),                                 # energy form, no layout launch (as up to 511 systems)
    ('atomic_layout1', dict(ATOMIC, **_layout(1))),           # energy form where the layout launch runs
    ('table_layout1', dict(TABLE, **_layout(1))),
    ('atomic_layout2', dict(ATOMIC, **_layout(2))),           # ... and hands every system back to its solve
    ('table_layout2', dict(TABLE, **_layout(2))),
    ('table_layout0', dict(TABLE, **_layout(0))),
    ('atomic_layout1_stream', dict(ATOMIC, UPSIDE_HIP_BP_COMPACT='0', **_layout(1))),     # the streaming solve ignores a pre-fold
    ('layout1_stream', dict(UPSIDE_HIP_BP_COMPACT='0', **_layout(1))),
    ('atomic_layout1_nolds', dict(ATOMIC, UPSIDE_HIP_BP_LDS_MSG_KB='0', **_layout(1))),   # every message in global memory: no LDS for the layout's scratch either, the streaming solve runs
    ('table_layout1_lds8', dict(TABLE, UPSIDE_HIP_BP_LDS_MSG_KB='8', **_layout(1))),      # the layout launch in front of a solve whose inbox leaves the LDS inside the rows to 3-state nodes
    ('atomic_cluster6', dict(ATOMIC, UPSIDE_HIP_BP_CLUSTER='6')),                         # the cluster solve in front of the hand-over launch
]


def expected_form(extra, n_system):
    """what `solve_form` of the side-chain node must report under BASE + extra: (p_prob, node_prob_in_solve, layout allocated, cluster > 1,
    layout word of every system, pre-fold taken over by the solve)"""
    env = dict(BASE, **extra)
    energy = 'UPSIDE_HIP_ROTAMER_ATOMIC' in env or 'UPSIDE_HIP_BP_ENERGY_TABLE' in env or int(env['UPSIDE_HIP_BP_CLUSTER']) > 1
    layout = int(env.get('UPSIDE_HIP_BP_LAYOUT', '-1'))
    allocated = layout >= 1 or (layout < 0 and n_system >= 512)
    cluster = int(env['UPSIDE_HIP_BP_CLUSTER']) > 1
    compact = env.get('UPSIDE_HIP_BP_COMPACT', '1') != '0'
    compact = compact and env.get('UPSIDE_HIP_BP_LDS_MSG_KB', '160') != '0'       # (the dense inbox borrows the LDS inbox for its scratch)
    runs = allocated and compact and not cluster            # k_rotamer_bp_layout is launched
    word = -1 if not runs else (1 if layout == 2 else 0)
    return dict(p_prob=0 if energy else 1, node_prob_in_solve=0, layout=int(allocated), cluster=int(cluster), word=word, compact=compact,
                prefold=int(runs and word == 0 and not energy))


def read_form(calc, engine, n_system):
    """the side-chain node's `solve_form` read-out as a dict (after a force evaluation)"""
    v = np.zeros(5 + n_system, 'f4')
    if calc.get_value_by_name(v.size, v.ctypes.data, engine, b'rotamer', b'solve_form'):
        raise RuntimeError('solve_form read-out failed')
    words = v[5:].astype(int)
    return dict(p_prob=int(v[0]), node_prob_in_solve=int(v[1]), layout=int(v[2]), cluster=int(v[3] > 1), select_prefold=int(v[4]),
                words=words)


def fold_condition(name, pos):
    """(active slot classes, multi-state nodes whose node_energy differs from their 1-body energy by > 1e-3) on the oracle.

    node_energy has the edges to 1-state partners folded in (rotamer.cpp:697-711); the 1-body energy of a state is the sum of its beads'
    entries in the probability nodes (rotamer.cpp:793-810), counted from the node's lowest state.  Nodes count in the order 1-state, 3-state, 6-state."""
    from upside_md_amd import h5lite
    with h5lite.open_file(P.fixture(name)) as t:
        g = t.group('input/potential/rotamer')
        args = [a.decode() if isinstance(a, bytes) else str(a) for a in g.get_attr('arguments')]
        ids = g.read('pair_interaction/id', 'i4').astype('u4')
        loc = g.read('pair_interaction/index', 'i4')
    orc = P.pkg.Upside(P.fixture(name), library=P.oracle_library())
    orc.energy(pos)
    n = int(orc.get_value_by_name((1,), 'rotamer', 'n_node')[0])
    ne = orc.get_value_by_name((n, 6), 'rotamer', 'node_energy').astype('f8')
    ee = orc.get_value_by_name((n, n, 6, 6), 'rotamer', 'edge_energy')
    one = np.zeros(len(ids))
    for a in args[1:]:
        one += orc.get_output(a)[loc, 0]
    orc.close()
    rot, n_rot, idx = ids & 15, (ids >> 4) & 15, ids >> 8
    n1 = int(idx[n_rot == 1].max()) + 1 if (n_rot == 1).any() else 0
    n3 = int(idx[n_rot == 3].max()) + 1 if (n_rot == 3).any() else 0
    start = {1: 0, 3: n1, 6: n1 + n3}
    node = np.array([start[int(k)] for k in n_rot]) + idx.astype(int)
    e1 = np.zeros((n, 6))
    np.add.at(e1, (node, rot.astype(int)), one)
    width = np.where(np.arange(n) < n1, 1, np.where(np.arange(n) < n1 + n3, 3, 6))
    valid = np.arange(6)[None, :] < width[:, None]
    e1 -= np.where(valid, e1, np.inf).min(axis=1)[:, None]         # convert_energy_to_prob takes each node's lowest state as its zero (rotamer.cpp:239-256)
    diff = np.where(valid, np.abs(ne - e1), 0.).max(axis=1)
    assert diff[width == 1].max(initial=0.) < 1e-5                   # (nothing is folded into a 1-state node: this reading of the 1-body energy is the oracle's)
    folded = int(((diff > 1e-3) & (width > 1)).sum())
    pair = (ee != 0).any(axis=(2, 3))
    cls = {}
    for (wa, wb) in ((1, 1), (3, 3), (3, 6), (6, 6)):
        cls['%dx%d' % (wa, wb)] = bool(pair[np.ix_(width == wa, width == wb)].any())
    cls['1xN'] = folded > 0           # (edge_energy does not list the edges to 1-state partners: the fold shows them)
    return cls, folded
