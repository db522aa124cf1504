"""GPU tests of the one replica-exchange procedure (energies summed on the device, upk_exchange_decide, one coordinate move) through
its callers: the engine's temperature sets (upside_hip_replica_swap_from / _next), its Hamiltonian sets (upside_hip_hamiltonian_swap),
the set over RCCL on a world of one, and the plain coordinate swaps.  Expectations are exact: verdicts that no uniform can change,
and coordinates compared bit for bit."""
import ctypes as ct
import numpy as np
import pytest
import parity_util as P

pytestmark = pytest.mark.gpu
E = P.pkg.engine
NAME = 'trpcage20_7A'
# the golden energies are 35.63 (pos) and 69.08 (pos2): across 0.01 | 100 the log-Boltzmann difference of trading them is -+3345.
# Cold system holding pos: exp(-3345) underflows to 0 and the pair is refused whatever the uniform; cold system holding pos2:
# +3345, accepted without a draw.
TEMPS = np.array([0.01, 100., 0.01, 100.], 'f4')
SET = np.array([[0, 1], [2, 3]], 'i4')


@pytest.fixture(scope='module')
def lib():
    import torch
    assert torch.cuda.is_available(), 'these tests need a GPU'
    lib = P.pkg.default_library()
    E.Ensemble._bind(lib.calc)
    for f in (lib.calc.upside_hip_replica_swap_from, lib.calc.upside_hip_replica_swap_next):
        f.argtypes = [ct.c_void_p, ct.c_int, ct.c_void_p, ct.c_uint32, ct.c_uint64, ct.c_int, ct.c_void_p]
    return lib


@pytest.fixture(scope='module')
def start():
    g = P.golden(NAME)
    assert float(g['energy2']) - float(g['energy']) > 30.      # what the verdicts below rest on
    return np.stack([g['pos'], g['pos2'], g['pos2'], g['pos']]).astype('f4')


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view('u4'), np.ascontiguousarray(b).view('u4'))


def four(lib, start, temps=TEMPS, files=False):
    ens = E.Ensemble.from_files([P.fixture(NAME)] * 4, library=lib) if files else E.Ensemble(P.fixture(NAME), 4, library=lib)
    ens.set_pos(start)
    ens.init_md(temps, 5)
    return ens


def swap_set(lib, ens, pairs, rnd, draw0=0, later=False):
    pairs = np.ascontiguousarray(pairs, 'i4')
    acc = np.full(len(pairs) + 1, -7, 'i4')
    fn = lib.calc.upside_hip_replica_swap_next if later else lib.calc.upside_hip_replica_swap_from
    return fn(ens.engine, len(pairs), pairs.ctypes.data, 99, rnd, draw0, acc.ctypes.data), acc


def test_temperature_set_with_mixed_verdicts(lib, start):
    ens = four(lib, start)
    rc, acc = swap_set(lib, ens, SET, 3)
    assert rc == 0
    assert list(acc) == [0, 1, 1]                              # one uniform drawn: for the rejectable pair only
    out = ens.get_pos()
    assert same_bits(out[0], start[0]) and same_bits(out[1], start[1])
    assert same_bits(out[2], start[3]) and same_bits(out[3], start[2])
    ens.close()


def test_hamiltonian_set_with_mixed_verdicts(lib, start):
    ens = four(lib, start, files=True)
    acc, draw = ens.hamiltonian_swap(SET, 99, 3, 0, want_accepted=True)
    assert list(acc) == [False, True] and draw == 1
    out = ens.get_pos()
    assert same_bits(out[0], start[0]) and same_bits(out[1], start[1])      # traded and traded back
    assert same_bits(out[2], start[3]) and same_bits(out[3], start[2])
    ens.close()


def test_overlapping_pairs_are_refused_and_move_nothing(lib, start):
    ens = four(lib, start)
    rc, _ = swap_set(lib, ens, [[0, 1], [1, 2]], 3)
    assert rc != 0
    assert same_bits(ens.get_pos(), start)
    ens.close()


@pytest.mark.parametrize('move', ['swap_systems', 'swap_system_pairs'])
def test_later_set_is_refused_after_a_coordinate_swap(lib, start, move):
    ens = four(lib, start, temps=np.full(4, 0.8, 'f4'))
    rc, acc = swap_set(lib, ens, SET, 3)
    assert rc == 0
    rc, acc = swap_set(lib, ens, [[1, 2]], 3, int(acc[-1]), later=True)      # the attempt's own swaps do not end it
    assert rc == 0
    if move == 'swap_systems':
        ens.swap_systems(0, 1)
    else:
        ens.swap_system_pairs([[0, 1]])
    rc, _ = swap_set(lib, ens, SET, 3, int(acc[-1]), later=True)
    assert rc != 0
    ens.close()


def test_later_set_over_rccl_is_refused_after_set_pos(lib, start):
    c = lib.calc
    temps = np.full(4, 0.8, 'f4')
    ens = four(lib, start, temps=temps)
    uid = ct.create_string_buffer(128)
    assert c.upside_hip_comm_get_unique_id(uid) == 0, c.upside_hip_last_error()
    assert c.upside_hip_comm_init(ens.engine, 0, 1, uid, temps.ctypes.data) == 0, c.upside_hip_last_error()
    acc = np.zeros(2, 'i4')
    later = np.array([[1, 2]], 'i4')
    assert c.upside_hip_comm_replica_swap(ens.engine, 2, SET.ctypes.data, 99, 3, 1, acc.ctypes.data) == 0, c.upside_hip_last_error()
    assert c.upside_hip_comm_replica_swap(ens.engine, 1, later.ctypes.data, 99, 3, 0, acc.ctypes.data) == 0, c.upside_hip_last_error()
    ens.set_pos(start)
    assert c.upside_hip_comm_replica_swap(ens.engine, 1, later.ctypes.data, 99, 3, 0, acc.ctypes.data) != 0
    c.upside_hip_comm_free(ens.engine)
    ens.close()


def test_swap_systems_is_swap_system_pairs_of_one_pair(lib, start):
    rs = np.random.RandomState(2)
    pos = (start + 0.01 * rs.normal(size=start.shape)).astype('f4')      # four distinct rows
    a, b = four(lib, pos), four(lib, pos)
    a.swap_systems(1, 2)
    b.swap_system_pairs([[1, 2]])
    xa, xb = a.get_pos(), b.get_pos()
    assert same_bits(xa, xb)
    assert same_bits(xa[0], pos[0]) and same_bits(xa[3], pos[3])
    assert same_bits(xa[1], pos[2]) and same_bits(xa[2], pos[1])
    a.close(); b.close()


def test_a_set_of_more_than_1024_pairs(lib):
    """1025 pairs: the smallest count above the limit the one-block swap kernel had.  Equal temperatures: lboltz_diff is exactly 0,
    every pair is accepted and no uniform is drawn."""
    n_pair = 1025
    g = P.golden(NAME)
    shift = (1e-3 * np.arange(2 * n_pair, dtype='f4'))[:, None, None]      # a rigid translation per system: distinct rows
    pos = (g['pos'].astype('f4')[None] + shift).astype('f4')
    ens = E.Ensemble(P.fixture(NAME), 2 * n_pair, library=lib)
    ens.set_pos(pos)
    ens.init_md(np.full(2 * n_pair, 0.8, 'f4'), 5)
    pairs = np.arange(2 * n_pair, dtype='i4').reshape(n_pair, 2)
    rc, acc = swap_set(lib, ens, pairs, 1)
    assert rc == 0
    assert np.all(acc[:n_pair] == 1) and acc[n_pair] == 0
    out = ens.get_pos()
    assert same_bits(out[0::2], pos[1::2]) and same_bits(out[1::2], pos[0::2])
    ens.close()


def test_an_empty_set_only_moves_the_draw_counter(lib, start):
    ens = four(lib, start, files=True)
    none = np.zeros((0, 2), 'i4')
    acc, draw = ens.hamiltonian_swap(none, 99, 3, 5, want_accepted=True)
    assert len(acc) == 0 and draw == 5
    acc, draw = ens.hamiltonian_swap(none, 99, 3, -1, want_accepted=True)      # continues from the counter the first call set
    assert draw == 5
    rc, acc = swap_set(lib, ens, none, 3, 7)
    assert rc == 0 and list(acc) == [7]
    assert same_bits(ens.get_pos(), start)
    ens.close()
