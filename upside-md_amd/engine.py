"""python3 ctypes mirror of the reference's `py/upside_engine.py` (`Upside` class, lines 159-242, and the
spline helpers, lines 93-156) over the engine_c_library C-ABI (/root/reference/src/engine_c_library.h:12-32).

`UpsideLibrary(path)` binds any shared object exporting that ABI: the HIP product
(`libupside_hip.so`), or -- in tests only -- the compiled reference under oracle/_ref.  The product
library is the default and there is NO fallback: if it cannot be loaded the import of
`default_library()` raises.
"""
import ctypes as ct
import os
import numpy as np
from . import h5lite

_HERE = os.path.dirname(os.path.abspath(__file__))
PRODUCT_LIB = os.path.join(_HERE, 'csrc', 'libupside_hip.so')


def _b(s):
    return s if isinstance(s, bytes) else str(s).encode()


class UpsideLibrary(object):
    def __init__(self, path):
        self.path = path
        # libhdf5 is a dependency of every engine build; load it first with RTLD_GLOBAL so a
        # library linked without an rpath still resolves it.
        try:
            h5lite.lib()
        except OSError:
            pass
        c = self.calc = ct.CDLL(path)
        c.construct_deriv_engine.restype = ct.c_void_p
        c.construct_deriv_engine.argtypes = [ct.c_int, ct.c_char_p, ct.c_bool]
        c.free_deriv_engine.restype = None
        c.free_deriv_engine.argtypes = [ct.c_void_p]
        for nm in ('evaluate_energy', 'evaluate_deriv'):
            getattr(c, nm).restype = ct.c_int
            getattr(c, nm).argtypes = [ct.c_void_p, ct.c_void_p, ct.c_void_p]
        for nm in ('set_param', 'get_param_deriv', 'get_param', 'get_sens', 'get_output'):
            getattr(c, nm).restype = ct.c_int
            getattr(c, nm).argtypes = [ct.c_int, ct.c_void_p, ct.c_void_p, ct.c_char_p]
        c.get_output_dims.restype = ct.c_int
        c.get_output_dims.argtypes = [ct.c_void_p, ct.c_void_p, ct.c_void_p, ct.c_char_p]
        c.get_value_by_name.restype = ct.c_int
        c.get_value_by_name.argtypes = [ct.c_int, ct.c_void_p, ct.c_void_p, ct.c_char_p, ct.c_char_p]
        c.get_clamped_value_and_deriv.restype = ct.c_int
        c.get_clamped_value_and_deriv.argtypes = [ct.c_int, ct.c_void_p, ct.c_void_p, ct.c_int, ct.c_void_p]
        c.clamped_spline_value.restype = ct.c_int
        c.clamped_spline_value.argtypes = [ct.c_int, ct.c_void_p, ct.c_void_p, ct.c_int, ct.c_void_p]
        c.clamped_spline_solve.restype = ct.c_int
        c.clamped_spline_solve.argtypes = [ct.c_int, ct.c_void_p, ct.c_void_p]
        c.get_clamped_coeff_deriv.restype = ct.c_int
        c.get_clamped_coeff_deriv.argtypes = [ct.c_int, ct.c_void_p, ct.c_void_p, ct.c_float]
        c.upside_main.restype = ct.c_int

    # -- free functions (upside_engine.py:93-156) ---------------------------------------------
    def clamped_spline_value(self, bspline_coeff, x):
        x = np.require(x, dtype='f4', requirements='C')
        bspline_coeff = np.require(bspline_coeff, dtype='f4', requirements='C')
        result = np.zeros(len(x), dtype='f4')
        if self.calc.clamped_spline_value(len(bspline_coeff), result.ctypes.data, bspline_coeff.ctypes.data,
                                          len(x), x.ctypes.data):
            raise RuntimeError("spline evaluation error")
        return result

    def clamped_spline_solve(self, values):
        values = np.require(values, dtype='f4', requirements='C')
        coeff = np.zeros(len(values) + 2, dtype='f4')
        if self.calc.clamped_spline_solve(len(coeff), coeff.ctypes.data, values.ctypes.data):
            raise RuntimeError("spline solve error")
        return coeff

    def clamped_value_and_deriv(self, bspline_coeff, x):
        x = np.require(x, dtype='f4', requirements='C')
        bspline_coeff = np.require(bspline_coeff, dtype='f4', requirements='C')
        result = np.zeros((len(x), 2), dtype='f4')
        if self.calc.get_clamped_value_and_deriv(len(bspline_coeff), result.ctypes.data,
                                                 bspline_coeff.ctypes.data, len(x), x.ctypes.data):
            raise RuntimeError("spline evaluation error")
        return result

    def clamped_coeff_deriv(self, bspline_coeff, x):
        x = np.asarray(x, dtype='f4')
        bspline_coeff = np.require(bspline_coeff, dtype='f4', requirements='C')
        result = np.zeros((len(x), len(bspline_coeff)), dtype='f4')
        for i, y in enumerate(x):
            if self.calc.get_clamped_coeff_deriv(len(bspline_coeff), result[i].ctypes.data,
                                                 bspline_coeff.ctypes.data, float(y)):
                raise RuntimeError("spline evaluation error")
        return result

    def in_process_upside(self, args, verbose=True):
        exec_args = [b'python_library', b'--re-raise-signal'] + [_b(a) for a in args]
        arr_t = ct.c_char_p * len(exec_args)
        arr = arr_t(*exec_args)
        self.calc.upside_main.argtypes = [ct.c_int, arr_t, ct.c_int]
        ret = self.calc.upside_main(len(exec_args), arr, int(verbose))
        if ret:
            raise RuntimeError('In process Upside returned %i' % ret)


_default = None


def default_library():
    """the HIP product library; raises if it has not been built (no CPU fallback)."""
    global _default
    if _default is None:
        if not os.path.exists(PRODUCT_LIB):
            raise RuntimeError('HIP extension %s is missing: run __graft_entry__.build()' % PRODUCT_LIB)
        _default = UpsideLibrary(PRODUCT_LIB)
    return _default


class Upside(object):
    """same method set as the reference's `Upside` (py/upside_engine.py:159-242)."""

    def __init__(self, config_file_path, quiet=True, library=None):
        self.lib = library if library is not None else default_library()
        self.calc = self.lib.calc
        self.config_file_path = str(config_file_path)
        with h5lite.open_file(self.config_file_path) as t:
            self.initial_pos = t.read('input/pos', 'f4')[:, :, 0]
            self.n_atom = self.initial_pos.shape[0]
            self.sequence = [x.decode() for x in t.read('input/sequence')] if 'input/sequence' in t else None
        self.engine = self.calc.construct_deriv_engine(self.n_atom, _b(self.config_file_path), bool(quiet))
        if not self.engine:
            raise RuntimeError('Unable to initialize upside engine for %s' % (config_file_path,))

    def __repr__(self):
        return 'Upside(%r, %r)' % (self.n_atom, self.config_file_path)

    def energy(self, pos):
        pos = np.require(pos, dtype='f4', requirements='C')
        assert pos.shape == (self.n_atom, 3)
        energy = np.zeros(1, dtype='f4')
        if self.calc.evaluate_energy(energy.ctypes.data, self.engine, pos.ctypes.data):
            raise RuntimeError('Unable to evaluate energy')
        return energy[0]

    def deriv(self, pos):
        pos = np.require(pos, dtype='f4', requirements='C')
        assert pos.shape == (self.n_atom, 3)
        deriv = np.zeros_like(pos)
        if self.calc.evaluate_deriv(deriv.ctypes.data, self.engine, pos.ctypes.data):
            raise RuntimeError('Unable to evaluate derivative')
        return deriv

    def set_param(self, param, node_name):
        param = np.require(np.asarray(param).ravel(), dtype='f4', requirements='C')
        if self.calc.set_param(int(param.shape[0]), param.ctypes.data, self.engine, _b(node_name)):
            raise RuntimeError('Unable to set param for node %s' % node_name)

    def get_param_deriv(self, param_shape, node_name):
        deriv = np.zeros(param_shape, dtype='f4')
        if self.calc.get_param_deriv(int(np.prod(param_shape)), deriv.ctypes.data, self.engine, _b(node_name)):
            raise RuntimeError('Unable to get param deriv')
        return deriv

    def get_param(self, param_shape, node_name):
        param = np.zeros(param_shape, dtype='f4')
        if self.calc.get_param(int(np.prod(param_shape)), param.ctypes.data, self.engine, _b(node_name)):
            raise RuntimeError('Unable to get param')
        return param

    def get_output_dims(self, node_name):
        n_elem = np.zeros(1, dtype=np.intc)
        elem_width = np.zeros(1, dtype=np.intc)
        if self.calc.get_output_dims(n_elem.ctypes.data, elem_width.ctypes.data, self.engine, _b(node_name)):
            raise RuntimeError('Unable to get output dims')
        return int(n_elem[0]), int(elem_width[0])

    def get_sens(self, node_name):
        shape = self.get_output_dims(node_name)
        out = np.zeros(shape, dtype='f4')
        if self.calc.get_sens(int(np.prod(shape)), out.ctypes.data, self.engine, _b(node_name)):
            raise RuntimeError('Unable to get sens')
        return out

    def get_output(self, node_name):
        shape = self.get_output_dims(node_name)
        out = np.zeros(shape, dtype='f4')
        if self.calc.get_output(int(np.prod(shape)), out.ctypes.data, self.engine, _b(node_name)):
            raise RuntimeError('Unable to get output')
        return out

    def get_value_by_name(self, value_shape, node_name, log_name):
        value = np.zeros(value_shape, dtype='f4')
        if self.calc.get_value_by_name(int(np.prod(value_shape)), value.ctypes.data, self.engine,
                                       _b(node_name), _b(log_name)):
            raise RuntimeError('Unable to get value by name')
        return value

    def close(self):
        if getattr(self, 'engine', None):
            self.calc.free_deriv_engine(self.engine)
            self.engine = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def unpack_walked_lists(node_name, system, side, info, cutoffs, sources, ints, floats):
    """the flat arrays of upside_hip_get_walked_lists (include/upside_engine_c.h) as a dict of named numpy arrays"""
    n_rows, n_other, cap = int(info[0]), int(info[1]), int(info[2])
    has_hit, has_hlo, has_ord, has_ordu = (bool(info[k]) for k in (9, 10, 11, 12))
    bits = int(info[7])
    src = (sources.split('\n') + ['', ''])[:2]
    r = dict(node=node_name, system=int(system), side=int(side), n_rows=n_rows, n_other=n_other, cap=cap,
             symmetric=bool(info[3]), md_sides=int(info[4]), itype=int(info[5]), word_bits=int(info[6]), nbr_j_bits=bits,
             n_slot=int(info[8]), upper=bool(info[16]), n_refine=int(info[17]), slot_none=int(info[18]), rebuilt=int(info[19]),
             cutoff=np.float32(cutoffs[0]), cache_cutoff=np.float32(cutoffs[1]), source_rows=src[0], source_other=src[1])
    at = [0]

    def take(a, n, shape=None):
        v = a[at[0]:at[0] + n].copy(); at[0] += n
        return v.reshape(shape) if shape else v
    r['cnt'] = take(ints, n_rows)
    r['hcnt'] = take(ints, n_rows) if has_hit else None
    r['hlo'] = take(ints, n_rows) if has_hlo else None
    r['ord'] = take(ints, n_rows) if has_ord else None
    r['ordu'] = take(ints, n_rows) if has_ordu else None
    for k, n in (('id_rows', n_rows), ('id_other', n_other), ('orig_rows', n_rows), ('orig_other', n_other),
                 ('loc_rows', n_rows), ('loc_other', n_other)):
        r[k] = take(ints, n)
    r['nbr_word'] = take(ints, n_rows * cap, (n_rows, cap))
    r['hit_word'] = take(ints, n_rows * cap, (n_rows, cap)) if has_hit else None
    assert at[0] == len(ints)
    mask = (1 << bits) - 1 if bits else -1
    for k in ('nbr', 'hit'):
        w = r[k + '_word']
        r[k] = None if w is None else (w & mask)
        r[k + '_slot'] = None if (w is None or not bits) else (w.view('u4') >> bits).astype('i4')
    at[0] = 0
    for k, n in (('cur_rows', n_rows), ('cur_other', n_other), ('cache_rows', n_rows), ('cache_other', n_other)):
        v = take(floats, n * 4, (n, 4))
        r[k] = v[:, :3].copy()
        if k.startswith('cache'):
            r[k.replace('cache', 'cache_id')] = v[:, 3].copy().view('i4')
    r['src_rows'] = take(floats, n_rows * 3, (n_rows, 3))
    r['src_other'] = take(floats, n_other * 3, (n_other, 3))
    assert at[0] == len(floats)
    return r


class Ensemble(object):
    """S systems of one topology resident on one GPU, driven through the `upside_hip_*` extension of the C-ABI
    (include/upside_engine_c.h): what `upside_main` does for its `systems` vector (main.cpp:441-700), with the
    state kept on the device between calls."""

    def __init__(self, config_file_path, n_system, device=None, quiet=True, library=None):
        self.lib = library if library is not None else default_library()
        c = self.calc = self.lib.calc
        self._bind(c)
        self.config_file_path = str(config_file_path)
        self.n_system = int(n_system)
        with h5lite.open_file(self.config_file_path) as t:
            self.initial_pos = t.read('input/pos', 'f4')[:, :, 0]
        self.n_atom = self.initial_pos.shape[0]
        if device is not None:
            self._check(c.upside_hip_set_device(int(device)), 'set_device')
        self.engine = c.upside_hip_construct(self.n_atom, _b(self.config_file_path), self.n_system, bool(quiet))
        if not self.engine:
            raise RuntimeError('Unable to initialize upside engine: %s' % c.upside_hip_last_error().decode())

    @classmethod
    def from_files(cls, paths, device=None, quiet=True, library=None):
        """one system per configuration file, in order (a file may repeat): a Hamiltonian ladder in one engine.  The files
        share their potential's structure; only the values of the per-system table may differ."""
        self = cls.__new__(cls)
        self.lib = library if library is not None else default_library()
        c = self.calc = self.lib.calc
        cls._bind(c)
        paths = [str(p) for p in paths]
        self.config_file_path = paths[0]
        self.config_file_paths = paths
        self.n_system = len(paths)
        with h5lite.open_file(paths[0]) as t:
            self.initial_pos = t.read('input/pos', 'f4')[:, :, 0]
        self.n_atom = self.initial_pos.shape[0]
        if device is not None:
            self._check(c.upside_hip_set_device(int(device)), 'set_device')
        arr = (ct.c_char_p * len(paths))(*[_b(p) for p in paths])
        self.engine = c.upside_hip_construct_files(self.n_atom, len(paths), arr, bool(quiet))
        if not self.engine:
            raise RuntimeError('Unable to initialize upside engine: %s' % c.upside_hip_last_error().decode())
        return self

    @staticmethod
    def _bind(c):
        if getattr(c, '_ensemble_bound', False):
            return
        vp, i32, u32, u64, f32 = ct.c_void_p, ct.c_int, ct.c_uint32, ct.c_uint64, ct.c_float
        c.upside_hip_set_device.argtypes = [i32]
        c.upside_hip_construct.restype = vp
        c.upside_hip_construct.argtypes = [i32, ct.c_char_p, i32, ct.c_bool]
        for nm in ('set_pos', 'get_pos', 'set_mom', 'get_mom'):
            getattr(c, 'upside_hip_' + nm).argtypes = [vp, vp]
        c.upside_hip_compute.argtypes = [vp, vp, vp]
        c.upside_hip_init_md.argtypes = [vp, vp, u32, f32, f32, i32]
        c.upside_hip_run_md.argtypes = [vp, i32]
        c.upside_hip_run_steps.argtypes = [vp, i32]
        c.upside_hip_recenter.argtypes = [vp]
        c.upside_hip_replica_swap.argtypes = [vp, i32, vp, u32, u64, vp]
        c.upside_replica_decide.argtypes = [i32, vp, vp, vp, u32, u64, i32, vp]
        c.upside_hip_get_system_pos.argtypes = [vp, i32, vp]
        c.upside_hip_set_system_pos.argtypes = [vp, i32, vp]
        c.upside_hip_swap_systems.argtypes = [vp, i32, i32]
        c.upside_hip_swap_system_pairs.argtypes = [vp, i32, vp]
        c.upside_hip_comm_get_unique_id.argtypes = [ct.c_char_p]
        c.upside_hip_comm_init.argtypes = [vp, i32, i32, ct.c_char_p, vp]
        c.upside_hip_comm_replica_swap.argtypes = [vp, i32, vp, u32, u64, i32, vp]
        c.upside_hip_comm_free.argtypes = [vp]
        c.upside_hip_get_param_deriv_all.argtypes = [vp, ct.c_char_p, i32, vp]
        c.upside_hip_param_deriv_accumulate.argtypes = [vp, ct.c_char_p, vp]
        c.upside_hip_param_deriv_read.argtypes = [vp, ct.c_char_p, i32, vp, vp, i32]
        c.upside_hip_construct_files.restype = vp
        c.upside_hip_construct_files.argtypes = [i32, i32, ct.POINTER(ct.c_char_p), ct.c_bool]
        c.upside_hip_group_configurations.argtypes = [i32, ct.POINTER(ct.c_char_p), vp]
        c.upside_hip_set_param_system.argtypes = [vp, ct.c_char_p, i32, i32, vp]
        c.upside_hip_get_param_system.argtypes = [vp, ct.c_char_p, i32, i32, vp]
        c.upside_hip_hamiltonian_swap.argtypes = [vp, i32, vp, u32, u64, i32, vp]
        c.upside_hip_last_error.restype = ct.c_char_p
        c.upside_hip_cv_define.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, vp]
        c.upside_hip_cv_define2.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, vp, vp]
        c.upside_hip_cv_define3.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        c.upside_hip_cv_load.argtypes = [vp, ct.c_char_p]
        c.upside_hip_cv_count.argtypes = [vp]
        c.upside_hip_cv_compute.argtypes = [vp, vp]
        c.upside_hip_cv_record.argtypes = [vp, i32, i32]
        c.upside_hip_cv_read.argtypes = [vp, i32, i32, vp, vp, vp, i32]
        c.upside_hip_cv_restraint_values.argtypes = [vp, ct.c_char_p, vp]
        c.upside_hip_metad_info.argtypes = [vp, ct.c_char_p, vp, vp, vp]
        c.upside_hip_metad_read.argtypes = [vp, ct.c_char_p, i32, vp, vp, vp, vp]
        c.upside_hip_metad_write.argtypes = [vp, ct.c_char_p, i32, vp, vp, i32]
        c.upside_hip_metad_values.argtypes = [vp, ct.c_char_p, vp]
        c.upside_hip_steer_info.argtypes = [vp, ct.c_char_p, vp]
        c.upside_hip_steer_read.argtypes = [vp, ct.c_char_p, vp, vp, vp]
        c.upside_hip_steer_write.argtypes = [vp, ct.c_char_p, vp, vp]
        c.upside_hip_steer_values.argtypes = [vp, ct.c_char_p, vp]
        c._ensemble_bound = True

    def _check(self, rc, what):
        if rc:
            raise RuntimeError('%s failed: %s' % (what, self.calc.upside_hip_last_error().decode()))

    # -- state ----------------------------------------------------------------------------------
    def set_pos(self, pos):
        pos = np.require(pos, dtype='f4', requirements='C')
        if pos.shape == (self.n_atom, 3):
            pos = np.ascontiguousarray(np.broadcast_to(pos, (self.n_system, self.n_atom, 3)))
        assert pos.shape == (self.n_system, self.n_atom, 3)
        self._check(self.calc.upside_hip_set_pos(self.engine, pos.ctypes.data), 'set_pos')

    def get_pos(self):
        out = np.zeros((self.n_system, self.n_atom, 3), 'f4')
        self._check(self.calc.upside_hip_get_pos(self.engine, out.ctypes.data), 'get_pos')
        return out

    def get_mom(self):
        out = np.zeros((self.n_system, self.n_atom, 3), 'f4')
        self._check(self.calc.upside_hip_get_mom(self.engine, out.ctypes.data), 'get_mom')
        return out

    def get_system_pos(self, system):
        out = np.zeros((self.n_atom, 3), 'f4')
        self._check(self.calc.upside_hip_get_system_pos(self.engine, int(system), out.ctypes.data), 'get_system_pos')
        return out

    def set_system_pos(self, system, pos):
        pos = np.require(pos, dtype='f4', requirements='C')
        assert pos.shape == (self.n_atom, 3)
        self._check(self.calc.upside_hip_set_system_pos(self.engine, int(system), pos.ctypes.data), 'set_system_pos')

    def swap_systems(self, s1, s2):
        self._check(self.calc.upside_hip_swap_systems(self.engine, int(s1), int(s2)), 'swap_systems')

    def swap_system_pairs(self, pairs):
        p = np.ascontiguousarray(np.asarray(pairs, 'i4').reshape(-1, 2))
        if len(p):
            self._check(self.calc.upside_hip_swap_system_pairs(self.engine, int(len(p)), p.ctypes.data), 'swap_system_pairs')

    # -- force pass / MD ------------------------------------------------------------------------
    def energies(self):
        e = np.zeros(self.n_system, 'f4')
        self._check(self.calc.upside_hip_compute(self.engine, e.ctypes.data, None), 'compute')
        return e

    def energies_and_derivs(self):
        e = np.zeros(self.n_system, 'f4'); d = np.zeros((self.n_system, self.n_atom, 3), 'f4')
        self._check(self.calc.upside_hip_compute(self.engine, e.ctypes.data, d.ctypes.data), 'compute')
        return e, d

    def init_md(self, temperature, base_seed, thermostat_timescale=5.0, dt=0.009, thermostat_interval=1):
        t = np.ascontiguousarray(np.broadcast_to(np.asarray(temperature, 'f4'), (self.n_system,)))
        self.temperature = t.copy()
        self._check(self.calc.upside_hip_init_md(self.engine, t.ctypes.data, int(base_seed) & 0xFFFFFFFF,
                                                 float(thermostat_timescale), float(dt), int(thermostat_interval)), 'init_md')

    def run_steps(self, n_step):
        self._check(self.calc.upside_hip_run_steps(self.engine, int(n_step)), 'run_steps')

    def run_rounds(self, n_round):
        self._check(self.calc.upside_hip_run_md(self.engine, int(n_round)), 'run_md')

    # -- parameters (set_param / get_param of the reference; per system for the nodes of the per-system table) -----------------
    def set_param(self, param, node_name, system=None):
        """system=None: every system (the reference's set_param); otherwise that system only"""
        p = np.require(np.asarray(param, 'f4').ravel(), dtype='f4', requirements='C')
        if system is None:
            self._check(self.calc.set_param(len(p), p.ctypes.data, self.engine, _b(node_name)), 'set_param')
        else:
            self._check(self.calc.upside_hip_set_param_system(self.engine, _b(node_name), int(system), len(p), p.ctypes.data), 'set_param_system')

    def get_param(self, shape, node_name, system=0):
        shape = tuple(shape)
        out = np.zeros(shape, 'f4')
        n = int(np.prod(shape, dtype=np.int64))
        if system == 0:      # (get_param: system 0's values, any node)
            self._check(self.calc.get_param(n, out.ctypes.data, self.engine, _b(node_name)), 'get_param')
        else:
            self._check(self.calc.upside_hip_get_param_system(self.engine, _b(node_name), int(system), n, out.ctypes.data), 'get_param_system')
        return out

    def hamiltonian_swap(self, pairs, base_seed, round_num, draw0=0, want_accepted=False):
        """one Hamiltonian swap set on the device (main.cpp:251-273): energy pass, pairs trade coordinates, energy pass,
        Metropolis verdicts at each system's own temperature, refused pairs trade back.  draw0 < 0 continues the draw counter
        of the previous set on the device.  want_accepted: (accepted as bool array, next draw) read back (synchronises);
        otherwise None and nothing waits."""
        p = np.ascontiguousarray(np.asarray(pairs, 'i4').reshape(-1, 2))
        acc = np.zeros(len(p) + 1, 'i4') if want_accepted else None
        self._check(self.calc.upside_hip_hamiltonian_swap(self.engine, int(len(p)), p.ctypes.data, int(base_seed) & 0xFFFFFFFF, int(round_num),
                                                          int(draw0), acc.ctypes.data if want_accepted else None), 'hamiltonian_swap')
        return (acc[:-1].astype(bool), int(acc[-1])) if want_accepted else None

    # -- parameter derivatives of every system (training: e.g. contrastive divergence) ----------------------------------
    # All three see the state of the LAST force pass (as get_param_deriv does): after set_pos or MD steps, call energies()
    # (or upside_hip_compute) first.  `shape` is the node's get_param() shape; () for a node without a derivative.
    def param_deriv(self, node_name, shape):
        """d(potential)/d(get_param of node_name) of every system: array (n_system,) + shape, deterministic"""
        shape = tuple(shape)
        out = np.zeros((self.n_system,) + shape, 'f4')
        self._check(self.calc.upside_hip_get_param_deriv_all(self.engine, _b(node_name), int(np.prod(shape, dtype=np.int64)) if shape else 0,
                                                             out.ctypes.data), 'get_param_deriv_all')
        return out

    def param_deriv_accumulate(self, node_name, weights=None):
        """enqueue sum[node] += sum_s weights[s] * param_deriv[s] on the device (weights: (n_system,), None = all 1, signed)"""
        w = None
        if weights is not None:
            w = np.ascontiguousarray(np.broadcast_to(np.asarray(weights, 'f4'), (self.n_system,)))
        self._check(self.calc.upside_hip_param_deriv_accumulate(self.engine, _b(node_name), None if w is None else w.ctypes.data),
                    'param_deriv_accumulate')

    def param_deriv_read(self, node_name, shape, reset=True):
        """(sum, n_frame): the accumulated float64 sum with the given shape and the number of accumulate calls since the last reset"""
        shape = tuple(shape)
        out = np.zeros(shape, 'f8')
        n = np.zeros(1, 'i8')
        self._check(self.calc.upside_hip_param_deriv_read(self.engine, _b(node_name), int(np.prod(shape, dtype=np.int64)) if shape else 0,
                                                          out.ctypes.data, n.ctypes.data, int(bool(reset))), 'param_deriv_read')
        return out, int(n[0])

    # -- collective variables of every system, on the device (kernels_cv.hip) --------------------------------------------
    def define_cvs(self, specs):
        """specs: the list of dicts config.add_collective_variables takes, or its packed form (the dict config.pack_collective_variables
        returns).  Replaces any earlier definition; [] clears it.  A refused definition raises and leaves the earlier one in force."""
        from . import config
        p = specs if isinstance(specs, dict) else config.pack_collective_variables(specs, self.n_atom)
        n_cv = len(p['kind'])
        arr = dict((k, np.ascontiguousarray(p[k], t)) for k, t in (('kind', 'i4'), ('atom_start', 'i4'), ('atoms', 'i4'), ('ref_pos', 'f4'),
                                                                     ('contact_r0', 'f4'), ('contact_beta', 'f4'), ('contact_lambda', 'f4')))
        dref = np.ascontiguousarray(p['dihedral_ref'], 'f4') if 'dihedral_ref' in p else None      # (a dict packed before the kind existed)
        path = [np.ascontiguousarray(p[k], t) if k in p else None for k, t in (('path_n_frame', 'i4'), ('path_lambda', 'f4'), ('path_ref_pos', 'f4'))]
        self._check(self.calc.upside_hip_cv_define3(self.engine, n_cv, *([arr[k].ctypes.data for k in
                    ('kind', 'atom_start', 'atoms', 'ref_pos', 'contact_r0', 'contact_beta', 'contact_lambda')] +
                    [None if v is None else v.ctypes.data for v in [dref] + path])), 'cv_define')
        self.cv_names = [x.decode() if isinstance(x, bytes) else str(x) for x in p['names']]
        self._cv_periods = config.cv_periods(p)

    def load_cvs(self, path=None):
        """/input/collective_variables of a configuration (default: the engine's own); returns the number of CVs (0: no such group)"""
        path = self.config_file_path if path is None else str(path)
        n = self.calc.upside_hip_cv_load(self.engine, _b(path))
        if n < 0:
            raise RuntimeError('cv_load failed: %s' % self.calc.upside_hip_last_error().decode())
        if n:
            from . import config
            with h5lite.open_file(path) as t:
                g = t.group('input').group('collective_variables')
                self.cv_names = [x.decode() for x in g.read('names').ravel()]
                self._cv_periods = config.cv_periods(dict(kind=g.read('kind')))
                del g      # (the handle is released before the file's)
        return n

    @property
    def cv_periods(self):
        """one period per CV of the current definition (2 pi for a dihedral, 0 = not periodic)"""
        return np.array(getattr(self, '_cv_periods', np.zeros(0)), 'f8')

    @property
    def n_cv(self):
        return int(self.calc.upside_hip_cv_count(self.engine))

    def cvs(self):
        """(n_system, n_cv) at the current device positions: one launch, no force pass"""
        out = np.zeros((self.n_system, self.n_cv), 'f4')
        self._check(self.calc.upside_hip_cv_compute(self.engine, out.ctypes.data), 'cv_compute')
        return out

    def record_cvs(self, every, capacity=0):
        """from now on every `every`-th completed MD round appends one (n_system, n_cv) sample to a device buffer of `capacity`
        samples, inside run_rounds / run_steps, with no host round trip; every=0 stops and frees the buffer"""
        self._check(self.calc.upside_hip_cv_record(self.engine, int(every), int(capacity)), 'cv_record')

    def cv_counts(self):
        """(n_stored, n_attempted) of the recording"""
        ns, na = np.zeros(1, 'i8'), np.zeros(1, 'i8')
        self._check(self.calc.upside_hip_cv_read(self.engine, 0, 0, None, ns.ctypes.data, na.ctypes.data, 0), 'cv_read')
        return int(ns[0]), int(na[0])

    def read_cvs(self, reset=True, with_counts=False):
        """the stored samples (n_stored, n_system, n_cv); with_counts: also (n_stored, n_attempted) -- more were due than stored when
        the buffer ran full.  reset empties the buffer (the round count, and with it the sampling phase, runs on)."""
        ns, na = self.cv_counts()
        out = np.zeros((ns, self.n_system, self.n_cv), 'f4')
        self._check(self.calc.upside_hip_cv_read(self.engine, 0, ns, out.ctypes.data, None, None, int(bool(reset))), 'cv_read')
        return (out, ns, na) if with_counts else out

    # -- diagnostics of the pair lists (read only) ----------------------------------------------
    def set_temperature(self, temperature):
        t = np.ascontiguousarray(np.broadcast_to(np.asarray(temperature, 'f4'), (self.n_system,)))
        self.calc.upside_hip_set_temperature.argtypes = [ct.c_void_p, ct.c_void_p]
        self._check(self.calc.upside_hip_set_temperature(self.engine, t.ctypes.data), 'set_temperature')
        self.temperature = t.copy()

    def rebuild_flags(self, node_name):
        """flags[s] = 1 where system s rebuilt the cached pair list of `node_name` in the last force pass"""
        fl = np.zeros(self.n_system, 'i4')
        self.calc.upside_hip_rebuild_flags.argtypes = [ct.c_void_p, ct.c_char_p, ct.c_void_p]
        self._check(self.calc.upside_hip_rebuild_flags(self.engine, _b(node_name), fl.ctypes.data), 'rebuild_flags')
        return fl

    def walked_lists(self, node_name, system, side):
        """what the pair passes of the last force pass walked for (node, system, side): a dict of numpy arrays (the layout of
        upside_hip_get_walked_lists, include/upside_engine_c.h, taken apart: `nbr` / `hit` hold the partner's element index,
        `nbr_slot` / `hit_slot` the slot field of a rotamer word, `nbr_word` / `hit_word` the words unchanged).  Raises
        RuntimeError with the library's reason, e.g. for a side the MD path does not keep (`.status` == 2)."""
        f = self.calc.upside_hip_get_walked_lists
        f.argtypes = [ct.c_void_p, ct.c_char_p, ct.c_int, ct.c_int, ct.c_void_p, ct.c_void_p, ct.c_char_p, ct.c_int,
                      ct.c_int, ct.c_void_p, ct.c_int, ct.c_void_p]
        info = np.zeros(20, 'i4'); cut = np.zeros(2, 'f4'); names = ct.create_string_buffer(512)

        def call(n_int, ints, n_float, floats):
            rc = f(self.engine, _b(node_name), int(system), int(side), info.ctypes.data, cut.ctypes.data, names, 512,
                   n_int, ints, n_float, floats)
            if rc:
                err = RuntimeError('walked_lists(%s, system %d, side %d): %s' % (
                    node_name, system, side, self.calc.upside_hip_last_error().decode()))
                err.status = rc
                raise err
        call(0, None, 0, None)
        ints = np.zeros(int(info[14]), 'i4'); floats = np.zeros(int(info[15]), 'f4')
        call(len(ints), ints.ctypes.data, len(floats), floats.ctypes.data)
        return unpack_walked_lists(node_name, system, side, info, cut, names.value.decode(), ints, floats)

    def backbone_list(self, node_name, system, must_have_list=True):
        """the cached residue-pair list of a backbone_pairs node for one system: dict(list_on, cap, skin, dist_cutoff, potential (the
        node's, of this system, in the last force pass that asked for energies), cnt, id, list [n_residue, cap], ref [n_residue, 3]:
        the reference centres the next force pass reads, centre: the current ones).  A node that keeps no list: RuntimeError
        (`.status` == 2), or with must_have_list=False the dict without the arrays and list_on False."""
        f = self.calc.upside_hip_get_backbone_list
        f.argtypes = [ct.c_void_p, ct.c_char_p, ct.c_int, ct.c_void_p, ct.c_void_p, ct.c_int, ct.c_void_p, ct.c_int, ct.c_void_p]
        info = np.zeros(2, 'i4'); cut = np.zeros(3, 'f4')

        def call(n_int, ints, n_float, floats):
            rc = f(self.engine, _b(node_name), int(system), info.ctypes.data, cut.ctypes.data, n_int, ints, n_float, floats)
            if rc and not (rc == 2 and not must_have_list):
                err = RuntimeError('backbone_list(%s, system %d): %s' % (node_name, system, self.calc.upside_hip_last_error().decode()))
                err.status = rc
                raise err
            return rc
        rc = call(0, None, 0, None)
        n, cap = int(info[0]), int(info[1])
        r = dict(node=node_name, system=int(system), side=0, list_on=rc == 0, n_residue=n, cap=cap)
        if rc == 0:
            ints = np.zeros(n * (2 + cap), 'i4'); floats = np.zeros(n * 7, 'f4')
            call(len(ints), ints.ctypes.data, len(floats), floats.ctypes.data)
            r.update(cnt=ints[:n].copy(), id=ints[n:2 * n].copy(), list=ints[2 * n:].reshape(n, cap).copy(),
                     ref=floats[:n * 4].reshape(n, 4)[:, :3].copy(), centre=floats[n * 4:].reshape(n, 3).copy())
        r.update(skin=np.float32(cut[0]), dist_cutoff=np.float32(cut[1]), potential=np.float32(cut[2]))
        return r

    def restraint_values(self, node_name):
        """(n_system, n_cv) CV values the cv_restraint node `node_name` saw in the last force pass (energies(), MD steps): the bits
        cvs() gives for the same definition at the same positions"""
        n_cv = int(self.calc.upside_hip_cv_restraint_values(self.engine, _b(node_name), None))      # (no out: the node's n_cv)
        out = np.zeros((self.n_system, max(n_cv, 0)), 'f4')
        if n_cv < 0 or self.calc.upside_hip_cv_restraint_values(self.engine, _b(node_name), out.ctypes.data) < 0:
            raise RuntimeError('cv_restraint_values failed: %s' % self.calc.upside_hip_last_error().decode())
        return out

    def umbrella_mbar(self, node_name, kT, tol=1e-8, max_iter=10000, f0=None, target=None, series=None, solver='self-consistent',
                      n_sc=10, uncertainty=False, decorrelate=False, n_bootstrap=0, bootstrap_seed=0, bootstrap_draw='host',
                      bootstrap_block=None, bootstrap_block_factor=5):
        """MBAR over the umbrella ladder of the cv_restraint node `node_name` from the recorded CV series (mbar.mbar on the device):
        system s is window s with its own row [center | spring_const | flat_width] (get_param of system s) and beta = 1 / kT for all
        (one temperature: the unbiased potential cancels and is not needed).  series: (n_stored, n_system, n_cv) as read_cvs gives it,
        default read_cvs(reset=False); sample (i, s) belongs to window s and every window counts n_stored samples.  The node's CVs
        are found among the recorded ones BY NAME (the names of the node's group against cv_names); a CV of the node that is not
        recorded raises ValueError naming it.  target: None, 'unbiased' (no bias at beta) or a row (3 n_cv,).  Returns the dict of
        mbar.mbar with values (N, d), rows (n_system, 3 d), periods (d,), n_k and names added; with a target, log_w feeds
        config.mbar_profile.  solver, n_sc: as mbar.mbar ('newton' for a ladder that converges slowly).  uncertainty=True adds sigma
        (n_system, n_system), the asymptotic standard deviation of f_i - f_j (mbar.free_energy_uncertainty: the samples are taken as
        uncorrelated, so pass decorrelate=True for a series recorded more often than its correlation time; it is a large-sample
        estimate, and n_bootstrap gives bootstrap error bars where few samples are kept or neighbours overlap poorly).
        decorrelate=True: per window, the series of its own-state reduced bias (mbar.own_state_reduced_bias) goes
        through timeseries.detect_equilibration on the device, the samples before the detected origin t0 are dropped and every
        ceil(g)-th of the rest is kept (timeseries.subsample_indices); MBAR and the uncertainty then run on the kept samples, window
        after window, with their unequal counts n_k, and t0, g, n_eff (each (n_system,)) and kept (the kept sample indices per
        window) are added to the result.  decorrelate=False changes nothing.  n_bootstrap > 0: that many stratified bootstrap
        replicates (mbar.bootstrap_counts with bootstrap_seed; every window keeps its sample count) are solved in one device batch
        from the returned f with the same tol and max_iter (mbar.bootstrap), and f_boot (n_bootstrap, n_system), sigma_boot
        (n_system, n_system) = mbar.bootstrap_sigma over the converged replicates, n_boot_converged and boot_counts (n_bootstrap, N)
        are added; the state every sample was drawn from follows the layout of values: sample (i, s) of window s without
        decorrelate, grouped by window with it.  Bootstrapping correlated samples underestimates the errors, so decorrelate=True
        goes with it -- or blocks: bootstrap_draw='device' draws the counts on the device (mbar.bootstrap(draw='device'), another
        stream of random numbers, no host array of counts), and bootstrap_block gives it the block lengths of the circular block
        bootstrap, which keeps every sample of a correlated series: an int, an (n_system,) array, or 'auto' =
        mbar.block_lengths(g, bootstrap_block_factor) with g the statistical inefficiency at origin 0
        (timeseries.statistical_inefficiency) of each window's own reduced bias, the series decorrelate forms.  'auto' with
        decorrelate=True raises ValueError (the kept samples are already uncorrelated), and so does a bootstrap_block with
        bootstrap_draw='host'.  With bootstrap_draw='device' the result holds boot_block (n_system,) (None without blocks) and
        boot_g ((n_system,) with 'auto', else None) and no boot_counts.  n_bootstrap=0 changes nothing, and a call without the
        bootstrap_draw and bootstrap_block options returns what it returned before them."""
        from . import config, mbar as _mbar
        if not (np.ndim(kT) == 0 and np.isfinite(kT) and kT > 0):
            raise ValueError('umbrella_mbar: kT must be one finite positive number (one temperature for every window)')
        if int(n_bootstrap) < 0:
            raise ValueError('umbrella_mbar: n_bootstrap must not be negative')
        if bootstrap_draw not in ('host', 'device'):
            raise ValueError("umbrella_mbar: bootstrap_draw must be 'host' or 'device', got %r" % (bootstrap_draw,))
        if bootstrap_block is not None and bootstrap_draw != 'device':
            raise ValueError("umbrella_mbar: bootstrap_block needs bootstrap_draw='device'")
        auto_block = isinstance(bootstrap_block, str)
        if auto_block and bootstrap_block != 'auto':
            raise ValueError("umbrella_mbar: bootstrap_block must be an int, an (n_system,) array or 'auto'")
        if auto_block and decorrelate:
            raise ValueError("umbrella_mbar: bootstrap_block='auto' with decorrelate=True: the kept samples are already uncorrelated")
        with h5lite.open_file(self.config_file_path) as t:
            pot = t.group('input').group('potential')
            if node_name not in pot:
                raise ValueError('umbrella_mbar: %s has no node %r' % (self.config_file_path, node_name))
            g = pot.group(node_name)
            names = [x.decode() for x in g.read('names').ravel()]
            periods = config.cv_periods(dict(kind=g.read('kind')))
            del g, pot
        recorded = list(getattr(self, 'cv_names', []))
        cols = []
        for nm in names:
            if nm not in recorded:
                raise ValueError('umbrella_mbar: the collective variable %r of node %r is not among the recorded ones %r' % (nm, node_name, recorded))
            cols.append(recorded.index(nm))
        d = len(names)
        rows = np.stack([self.get_param((3 * d,), node_name, system=s) for s in range(self.n_system)])
        if series is None:
            series = self.read_cvs(reset=False)
        series = np.asarray(series, 'f4')
        if series.ndim != 3 or series.shape[1] != self.n_system or series.shape[2] != len(recorded):
            raise ValueError('umbrella_mbar: the series must be (n_stored, %d systems, %d CVs), got %r' % (self.n_system, len(recorded), series.shape))
        values = np.ascontiguousarray(series[:, :, cols].reshape(-1, d))
        n_k = np.full(self.n_system, series.shape[0], 'i8')
        beta = 1. / float(kT)
        extra = {}
        if decorrelate:
            from . import timeseries as _ts
            per_window = np.ascontiguousarray(series[:, :, cols].transpose(1, 0, 2))      # (n_system, n_stored, d)
            state = np.repeat(np.arange(self.n_system), series.shape[0])
            bias = _mbar.own_state_reduced_bias(per_window.reshape(-1, d), beta, rows, periods, state).reshape(self.n_system, -1)
            t0, g, n_eff = _ts.detect_equilibration(bias, library=self.lib)
            kept = [_ts.subsample_indices(series.shape[0], t0[s], g[s]) for s in range(self.n_system)]
            values = np.ascontiguousarray(np.concatenate([per_window[s][kept[s]] for s in range(self.n_system)]))
            n_k = np.array([len(k) for k in kept], 'i8')
            extra = dict(t0=t0, g=g, n_eff=n_eff, kept=kept)
        if isinstance(target, str):
            if target != 'unbiased':
                raise ValueError("umbrella_mbar: target must be None, 'unbiased' or a row")
            tgt = (beta, None)
        else:
            tgt = None if target is None else (beta, target)
        out = _mbar.mbar(values, None, beta, rows, n_k, periods, tol, max_iter, f0=f0, target=tgt, library=self.lib, solver=solver, n_sc=n_sc)
        if uncertainty:
            out['sigma'] = _mbar.free_energy_uncertainty(values, None, beta, rows, n_k, out['f'], periods, library=self.lib)
        if int(n_bootstrap) > 0:
            import warnings
            origin = np.repeat(np.arange(self.n_system), n_k) if decorrelate else np.tile(np.arange(self.n_system), series.shape[0])
            boot_g, block = None, bootstrap_block
            if auto_block:
                from . import timeseries as _ts
                per_window = np.ascontiguousarray(series[:, :, cols].transpose(1, 0, 2))      # (n_system, n_stored, d)
                state = np.repeat(np.arange(self.n_system), series.shape[0])
                bias = _mbar.own_state_reduced_bias(per_window.reshape(-1, d), beta, rows, periods, state).reshape(self.n_system, -1)
                boot_g = np.asarray(_ts.statistical_inefficiency(bias, library=self.lib)['g'], 'f8').reshape(-1)
                block = _mbar.block_lengths(boot_g, bootstrap_block_factor)
            boot = _mbar.bootstrap(values, None, beta, rows, n_k, out['f'], origin, int(n_bootstrap), bootstrap_seed, periods=periods, tol=tol,
                                   max_iter=max_iter, library=self.lib, draw=bootstrap_draw, block=block)
            with warnings.catch_warnings():      # (the number of unconverged replicates is returned below)
                warnings.simplefilter('ignore', RuntimeWarning)
                sigma_boot = _mbar.bootstrap_sigma(boot)
            extra.update(f_boot=boot['f_boot'], sigma_boot=sigma_boot, n_boot_converged=int(boot['converged'].sum()))
            if bootstrap_draw == 'device':
                extra.update(boot_block=boot['block'], boot_g=boot_g)
            else:
                extra.update(boot_counts=boot['counts'])
        out.update(values=values, rows=rows, periods=periods, n_k=n_k, names=names, **extra)
        return out

    # -- cv_metadynamics: the hills of a node (they live on the device; deposition happens inside run_rounds / run_steps) -----
    def metad_info(self, node_name):
        """(d, capacity, n_list) of the cv_metadynamics node: n_list is n_system (shared = 0) or 1 (shared = 1)"""
        v = np.zeros(3, 'i4')
        self._check(self.calc.upside_hip_metad_info(self.engine, _b(node_name), v[0:].ctypes.data, v[1:].ctypes.data, v[2:].ctypes.data), 'metad_info')
        return int(v[0]), int(v[1]), int(v[2])

    def _metad_list(self, node_name, system):
        d, cap, n_list = self.metad_info(node_name)
        if not 0 <= int(system) < self.n_system:
            raise ValueError('system %r out of range' % (system,))
        return d, cap, (int(system) if n_list > 1 else 0)      # (a shared list serves every system)

    def metad_hills(self, node_name, system=0):
        """(centers (n, d) f4, weights (n,) f4, n_attempt): the hills system `system` sees (its own list, or the shared one in walker
        order: deposit k of system s is row k * n_system + s) and the deposits attempted so far; n_attempt beyond the deposits
        stored means the list ran full"""
        d, cap, lst = self._metad_list(node_name, system)
        c = np.zeros((cap, d), 'f4'); w = np.zeros(cap, 'f4'); n = np.zeros(1, 'i4'); na = np.zeros(1, 'i8')
        self._check(self.calc.upside_hip_metad_read(self.engine, _b(node_name), lst, c.ctypes.data, w.ctypes.data, n.ctypes.data, na.ctypes.data), 'metad_read')
        return c[:n[0]].copy(), w[:n[0]].copy(), int(na[0])

    def set_metad_hills(self, node_name, centers, weights, system=0):
        """replace the list system `system` sees by these hills (centers (n, d) or (n,) for d = 1, weights (n,)); deposition
        continues after them.  Stream-ordered: the next force pass sees them, also from a captured graph."""
        d, cap, lst = self._metad_list(node_name, system)
        w = np.require(np.asarray(weights, 'f4').reshape(-1), dtype='f4', requirements='C')
        c = np.require(np.asarray(centers, 'f4').reshape(len(w), d), dtype='f4', requirements='C')
        self._check(self.calc.upside_hip_metad_write(self.engine, _b(node_name), lst, c.ctypes.data, w.ctypes.data, len(w)), 'metad_write')

    def metad_values(self, node_name):
        """(n_system, d) CV values the cv_metadynamics node saw in the last force pass: the bits cvs() gives for the same
        definition at the same positions"""
        d = self.metad_info(node_name)[0]
        out = np.zeros((self.n_system, d), 'f4')
        self._check(self.calc.upside_hip_metad_values(self.engine, _b(node_name), out.ctypes.data), 'metad_values')
        return out

    def metad_reweight(self, node_name, kT, axes=None, series=None, every=1, first_round=0, max_checkpoints=4096):
        """the reweighting of the recorded frames of a metadynamics run (metad.frame_log_weights on the device; Tiwary & Parrinello
        2015): the hills come from metad_hills, pace, kdT, sigma and shared from the node's group in config_file_path, the frames
        from series ((n_stored, n_system, n_cv) as read_cvs gives it, default read_cvs(reset=False)).  The node's CVs are found among
        the recorded ones BY NAME; a CV of the node that is not recorded raises ValueError naming it.  Frame i was recorded at
        completed round first_round + (i + 1) * every, counted from the start of the deposits (record_cvs(every) called before the
        first round gives first_round = 0).  axes: the d grid axes c(t) is integrated over, default metad.default_axes over all the
        hills.  Returns the dict of metad.frame_log_weights per system (a list of n_system dicts; each system has its own list of
        hills and its own weights, all of them from one bias call and one grid call), or, for a shared list, ONE dict over the
        pooled frames in the order of series.reshape(-1, d) (frame-major, n_walker = n_system); `axes` is added to every dict."""
        from . import config, metad as _metad
        p = config.metad_node_parameters(self.config_file_path, node_name)
        recorded = list(getattr(self, 'cv_names', []))
        cols = []
        for nm in p['names']:
            if nm not in recorded:
                raise ValueError('metad_reweight: the collective variable %r of node %r is not among the recorded ones %r' % (nm, node_name, recorded))
            cols.append(recorded.index(nm))
        d = len(cols)
        if int(every) < 1 or int(first_round) < 0:
            raise ValueError('metad_reweight: every >= 1 and first_round >= 0')
        if series is None:
            series = self.read_cvs(reset=False)
        series = np.asarray(series, 'f4')
        if series.ndim != 3 or series.shape[1] != self.n_system or series.shape[2] != len(recorded) or not series.shape[0]:
            raise ValueError('metad_reweight: the series must be (n_stored >= 1, %d systems, %d CVs), got %r' % (self.n_system, len(recorded), series.shape))
        n = series.shape[0]
        rounds = int(first_round) + (np.arange(n, dtype='i8') + 1) * int(every)
        S = self.n_system
        if p['shared']:
            c, w, _ = self.metad_hills(node_name, 0)
            if not len(w):
                raise ValueError('metad_reweight: node %r holds no hills yet' % node_name)
            axes = _metad.default_axes(c, p['sigma'], p['periods']) if axes is None else axes
            out = _metad.frame_log_weights(c, w, p['sigma'], series[:, :, cols].reshape(-1, d), np.repeat(rounds, S), p['pace'], kT, p['kdT'], axes,
                                           n_walker=S, periods=p['periods'], max_checkpoints=max_checkpoints, library=self.lib)
            out['axes'] = axes
            return out
        lists = [self.metad_hills(node_name, s)[:2] for s in range(S)]
        c = np.concatenate([l[0] for l in lists]); w = np.concatenate([l[1] for l in lists])
        if not len(w):
            raise ValueError('metad_reweight: node %r holds no hills yet' % node_name)
        hs = np.concatenate(([0], np.cumsum([len(l[1]) for l in lists]))).astype('i8')
        axes = _metad.default_axes(c, p['sigma'], p['periods']) if axes is None else axes
        frames = np.ascontiguousarray(series[:, :, cols].transpose(1, 0, 2)).reshape(-1, d)      # (system-major: the frames of a list together)
        out = _metad.frame_log_weights_lists(c, w, p['sigma'], frames, np.tile(rounds, S), p['pace'], kT, p['kdT'], axes, hs, n * np.arange(S + 1),
                                             periods=p['periods'], max_checkpoints=max_checkpoints, library=self.lib)
        for o in out:
            o['axes'] = axes
        return out

    # -- cv_steer: clocks, work and centres of a node (they live on the device and advance inside run_rounds / run_steps) ---------
    def _steer_n_cv(self, node_name):
        n = np.zeros(1, 'i4')
        self._check(self.calc.upside_hip_steer_info(self.engine, _b(node_name), n.ctypes.data), 'steer_info')
        return int(n[0])

    def steer_state(self, node_name):
        """dict(clock (n_system,) i8: completed MD rounds since the clock was last set; work (n_system,) f8: the accumulated work of
        moving the centres; center (n_system, n_cv) f8: the centres in force, as of the last force pass or completed round).  Work
        and clock belong to the system index: a coordinate swap leaves them where they are."""
        n_cv = self._steer_n_cv(node_name)
        clock = np.zeros(self.n_system, 'i8'); work = np.zeros(self.n_system, 'f8'); center = np.zeros((self.n_system, n_cv), 'f8')
        self._check(self.calc.upside_hip_steer_read(self.engine, _b(node_name), clock.ctypes.data, work.ctypes.data, center.ctypes.data), 'steer_read')
        return dict(clock=clock, work=work, center=center)

    def set_steer_state(self, node_name, clock=None, work=None):
        """replace the clocks and / or the work of every system (a scalar or (n_system,); None: kept).  Stream-ordered: the next
        force pass sees them, also from a captured graph."""
        self._steer_n_cv(node_name)
        ck = None if clock is None else np.ascontiguousarray(np.broadcast_to(np.asarray(clock, 'i8'), (self.n_system,)))
        wk = None if work is None else np.ascontiguousarray(np.broadcast_to(np.asarray(work, 'f8'), (self.n_system,)))
        self._check(self.calc.upside_hip_steer_write(self.engine, _b(node_name), None if ck is None else ck.ctypes.data,
                                                     None if wk is None else wk.ctypes.data), 'steer_write')

    def steer_values(self, node_name):
        """(n_system, n_cv) CV values the cv_steer node saw in the last force pass: the bits cvs() gives for the same definition at the
        same positions"""
        out = np.zeros((self.n_system, self._steer_n_cv(node_name)), 'f4')
        self._check(self.calc.upside_hip_steer_values(self.engine, _b(node_name), out.ctypes.data), 'steer_values')
        return out

    # -- replica exchange across the engines of a job, inside the library (comm_rccl.cpp) -------------
    COMM_ID_BYTES = 128

    def comm_unique_id(self):
        """rank 0: the rendezvous token every rank passes to comm_init (hand it around with any host channel)"""
        uid = ct.create_string_buffer(self.COMM_ID_BYTES)
        self._check(self.calc.upside_hip_comm_get_unique_id(uid), 'comm_get_unique_id')
        return uid.raw

    def comm_init(self, rank, world, unique_id, temperature_global):
        """joins this engine (rank `rank` of `world`, equal system counts) to the exchange group; temperature_global:
        the whole ladder, rank r owns entries [r*n_system, (r+1)*n_system)"""
        t = np.ascontiguousarray(np.asarray(temperature_global, 'f4'))
        assert t.shape == (int(world) * self.n_system,)
        uid = ct.create_string_buffer(bytes(unique_id), self.COMM_ID_BYTES)
        self._check(self.calc.upside_hip_comm_init(self.engine, int(rank), int(world), uid, t.ctypes.data), 'comm_init')

    def comm_replica_swap(self, pairs_global, base_seed, round_num, first_set, want_accepted=False):
        """one swap set over GLOBAL replica indices: energies all-gathered over RCCL (first set of an attempt only),
        Metropolis verdicts on the device, coordinates of accepted pairs traded (ncclSend/ncclRecv when they straddle
        ranks).  Everything is enqueued behind the MD steps; want_accepted reads the verdicts back (synchronises)."""
        p = np.ascontiguousarray(np.asarray(pairs_global, 'i4').reshape(-1, 2))
        acc = np.zeros(len(p), 'i4') if want_accepted else None
        self._check(self.calc.upside_hip_comm_replica_swap(self.engine, int(len(p)), p.ctypes.data, int(base_seed) & 0xFFFFFFFF,
                                                           int(round_num), int(bool(first_set)),
                                                           acc.ctypes.data if want_accepted else None), 'comm_replica_swap')
        return acc.astype(bool) if want_accepted else None

    def close(self):
        if getattr(self, 'engine', None):
            self.calc.free_deriv_engine(ct.c_void_p(self.engine))
            self.engine = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


BatchEngine = Ensemble      # the batched engine under the name the documents use


def group_configurations(paths, library=None):
    """the grouping upside_main uses (HDF5 only, no GPU): group index of every file, numbered by first appearance.  Files that
    are identical or differ only in the values of the per-system table share a group."""
    lib = library if library is not None else default_library()
    Ensemble._bind(lib.calc)
    paths = [str(p) for p in paths]
    arr = (ct.c_char_p * len(paths))(*[_b(p) for p in paths])
    out = np.zeros(len(paths), 'i4')
    if lib.calc.upside_hip_group_configurations(len(paths), arr, out.ctypes.data) < 0:
        raise RuntimeError('group_configurations failed: %s' % lib.calc.upside_hip_last_error().decode())
    return out


def replica_decide(pairs, beta, energy, base_seed, round_num, draw0=0, library=None):
    """Metropolis verdicts of one swap set from known energies (host arithmetic of main.cpp:251-273; needs no GPU).
    Returns (accepted[n_pair] as bool array, next draw index)."""
    lib = library if library is not None else default_library()
    Ensemble._bind(lib.calc)
    pairs = np.require(pairs, dtype='i4', requirements='C').reshape(-1, 2)
    beta = np.require(beta, dtype='f4', requirements='C')
    energy = np.require(energy, dtype='f4', requirements='C')
    if pairs.size and (pairs.min() < 0 or pairs.max() >= len(energy) or len(beta) != len(energy)):
        raise ValueError('swap pairs outside the system list')
    acc = np.zeros(len(pairs) + 1, 'i4')
    if lib.calc.upside_replica_decide(len(pairs), pairs.ctypes.data, beta.ctypes.data, energy.ctypes.data,
                                      int(base_seed) & 0xFFFFFFFF, int(round_num), int(draw0), acc.ctypes.data):
        raise RuntimeError('replica_decide failed')
    return acc[:-1].astype(bool), int(acc[-1])
