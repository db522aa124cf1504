"""Pairwise RMSD of frames on the device and the clusterings built on it (upside_hip_frames_create, upside_hip_rmsd_matrix, _nearest,
_count of include/upside_engine_c.h; csrc/kernels_rmsd.hip).  For frames a, b of n atoms, centred each on its own centroid in fp64,
    d2_ab = max(0, G_a + G_b - 2 lambda_ab) / n      d_ab = sqrt(d2_ab)
with G_f = sum_i |y_f,i|^2 and lambda_ab the largest eigenvalue of Horn's 4 x 4 matrix of M_ab = sum_i y_a,i y_b,i^T: the RMSD after
the best PROPER rotation (no reflection), all atoms with equal weight, as the `rmsd` collective variable.  A Frames object holds the
centred coordinates on the device; every call names frame sets plus optional index lists of positions into them (repeats allowed).
Limits: n_atom >= 3; distances below about 1e-6 sqrt((G_a + G_b) / n) are rounding noise (two copies of a frame come out near
1e-7 A, not 0, except on the diagonal of a symmetric matrix, which is exactly 0); a set holds 3 F n_pad doubles on the device (n_pad =
n_atom rounded up to 4: 4.2 GB for 2^20 frames of 168 atoms); the full matrix needs nA nB doubles on the device and the host -- above
that nearest, count_within and gromos are the route, which never store it; one device."""
import ctypes as ct
import numpy as np


def _bind(c):
    if getattr(c, '_rmsd_bound', False):
        return
    vp, i32, i64 = ct.c_void_p, ct.c_int, ct.c_longlong
    c.upside_hip_frames_create.argtypes = [i32, i64, vp, vp]
    c.upside_hip_frames_create.restype = i32
    c.upside_hip_frames_free.argtypes = [vp]
    c.upside_hip_frames_free.restype = None
    c.upside_hip_rmsd_matrix.argtypes = [vp, i64, vp, vp, i64, vp, vp]
    c.upside_hip_rmsd_matrix.restype = i32
    c.upside_hip_rmsd_nearest.argtypes = [vp, i64, vp, vp, i64, vp, vp, vp]
    c.upside_hip_rmsd_nearest.restype = i32
    c.upside_hip_rmsd_count.argtypes = [vp, i64, vp, vp, i64, vp, ct.c_double, vp]
    c.upside_hip_rmsd_count.restype = i32
    c.upside_hip_last_error.restype = ct.c_char_p
    c._rmsd_bound = True


def _library(library):
    from .engine import default_library
    lib = library if library is not None else default_library()
    _bind(lib.calc)
    return lib.calc


def select_atoms(pos, atoms=None):
    """pos (F, n_atom, 3) as contiguous float32 with the optional index list `atoms` applied; the checks of Frames"""
    x = np.asarray(pos)
    if x.ndim != 3 or x.shape[2] != 3:
        raise ValueError('cluster: pos must be (F, n_atom, 3), got %r' % (x.shape,))
    if atoms is not None:
        at = np.asarray(atoms).reshape(-1)
        if at.dtype.kind not in 'iu' or not len(at):
            raise ValueError('cluster: atoms must be a list of whole numbers, at least one')
        if at.min() < 0 or at.max() >= x.shape[1]:
            raise ValueError('cluster: atoms must lie in 0 .. %d' % (x.shape[1] - 1))
        x = x[:, at]
    if x.shape[0] < 1:
        raise ValueError('cluster: at least one frame is needed')
    if x.shape[1] < 3:
        raise ValueError('cluster: %d atoms per frame, at least 3 are needed' % x.shape[1])
    x = np.ascontiguousarray(x, 'f4')
    if not np.isfinite(x).all():
        bad = int(np.argwhere(~np.isfinite(x).all(axis=(1, 2)))[0, 0])
        raise ValueError('cluster: frame %d holds a coordinate that is not finite' % bad)
    return x


class Frames:
    """F frames of n_atom atoms on the device, centred in fp64.  pos (F, n_atom, 3) (float32 as get_pos() and /output/pos deliver;
    anything else is rounded to float32); atoms: an optional index list applied on the host first, e.g. every third atom for C-alpha.
    Creation is the only copy of coordinates to the device.  A context manager; close() frees the device memory."""

    def __init__(self, pos, atoms=None, library=None):
        self._handle = None
        x = select_atoms(pos, atoms)
        self.n_frame, self.n_atom = int(x.shape[0]), int(x.shape[1])
        self._lib = _library(library)
        h = ct.c_void_p()
        if self._lib.upside_hip_frames_create(self.n_atom, self.n_frame, x.ctypes.data, ct.byref(h)):
            raise RuntimeError('cluster.Frames failed: %s' % self._lib.upside_hip_last_error().decode())
        self._handle = h

    def __len__(self):
        return self.n_frame

    def close(self):
        if self._handle is not None:
            self._lib.upside_hip_frames_free(self._handle)
            self._handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        self.close()


class _Wrapped:
    """a Frames as it is, or an array wrapped for one call"""

    def __init__(self, x, atoms, library, what):
        self.own = not isinstance(x, Frames)
        if self.own:
            self.f = Frames(x, atoms, library)
        else:
            if atoms is not None:
                raise ValueError('cluster: atoms applies to arrays; %s is a Frames, which was made with its own' % what)
            if x._handle is None:
                raise ValueError('cluster: %s is a closed Frames' % what)
            self.f = x

    def close(self):
        if self.own:
            self.f.close()


def _positions(idx, frames, what):
    """(n, int32 array or None)"""
    if idx is None:
        return frames.n_frame, None
    i = np.asarray(idx)
    if i.ndim != 1 or not len(i) or i.dtype.kind not in 'iu':
        raise ValueError('cluster: %s must be a list of whole numbers, at least one' % what)
    if i.min() < 0 or i.max() >= frames.n_frame:
        raise ValueError('cluster: %s must lie in 0 .. %d' % (what, frames.n_frame - 1))
    i = np.ascontiguousarray(i, 'i4')
    return len(i), i


def _sides(a, b, ia, ib, atoms, library):
    A = _Wrapped(a, atoms, library, 'a')
    try:
        if b is None or b is a:
            B = A
            if b is None and ib is None:
                ib = ia
        else:
            B = _Wrapped(b, atoms, library, 'b')
        try:
            if A.f.n_atom != B.f.n_atom:
                raise ValueError('cluster: the frames of a hold %d atoms, those of b %d' % (A.f.n_atom, B.f.n_atom))
            nA, ia = _positions(ia, A.f, 'ia')
            nB, ib = _positions(ib, B.f, 'ib')
        except Exception:
            if B is not A:
                B.close()
            raise
    except Exception:
        A.close()
        raise
    return A, B, nA, ia, nB, ib


def _done(A, B):
    if B is not A:
        B.close()
    A.close()


def _p(a):
    return None if a is None else a.ctypes.data


def rmsd_matrix(a, b=None, ia=None, ib=None, atoms=None, library=None):
    """(nA, nB) float64: d of row position p and column position q.  a, b: Frames or (F, n_atom, 3) arrays (wrapped for the call, with
    `atoms` applied); b None: a against itself with the same index list -- only pairs p < q are computed, the matrix is bitwise
    symmetric and its diagonal exactly 0.  ia, ib: positions into the sets (repeats allowed), None: all frames in order.  Shape and
    value errors raise ValueError before the library is touched; a refusal of the library raises RuntimeError with its message."""
    A, B, nA, ia, nB, ib = _sides(a, b, ia, ib, atoms, library)
    try:
        if nA * nB >= 1 << 40:
            raise ValueError('cluster.rmsd_matrix: %d x %d entries, fewer than 2^40 are supported' % (nA, nB))
        out = np.zeros((nA, nB), 'f8')
        lib = A.f._lib
        if lib.upside_hip_rmsd_matrix(A.f._handle, nA, _p(ia), B.f._handle, nB, _p(ib), out.ctypes.data):
            raise RuntimeError('cluster.rmsd_matrix failed: %s' % lib.upside_hip_last_error().decode())
        return out
    finally:
        _done(A, B)


def nearest(a, b, ia=None, ib=None, atoms=None, library=None):
    """(index (nA,) int64, dist (nA,) float64): for every row position the column POSITION with the smallest d2 (the lowest on equal
    bits) and that d.  Arguments and errors as rmsd_matrix; the pair matrix is never stored."""
    if b is None:
        raise ValueError('cluster.nearest: b must be given')
    A, B, nA, ia, nB, ib = _sides(a, b, ia, ib, atoms, library)
    try:
        index = np.zeros(nA, 'i8'); dist = np.zeros(nA, 'f8')
        lib = A.f._lib
        if lib.upside_hip_rmsd_nearest(A.f._handle, nA, _p(ia), B.f._handle, nB, _p(ib), index.ctypes.data, dist.ctypes.data):
            raise RuntimeError('cluster.nearest failed: %s' % lib.upside_hip_last_error().decode())
        return index, dist
    finally:
        _done(A, B)


def count_within(a, b, cutoff, ia=None, ib=None, atoms=None, library=None):
    """(nA,) int64: for every row position the number of column positions with d2 <= cutoff^2.  Arguments and errors as nearest."""
    if b is None:
        raise ValueError('cluster.count_within: b must be given')
    if not (np.ndim(cutoff) == 0 and np.isfinite(cutoff) and cutoff >= 0):
        raise ValueError('cluster.count_within: cutoff must be one finite number, not negative')
    A, B, nA, ia, nB, ib = _sides(a, b, ia, ib, atoms, library)
    try:
        count = np.zeros(nA, 'i8')
        lib = A.f._lib
        if lib.upside_hip_rmsd_count(A.f._handle, nA, _p(ia), B.f._handle, nB, _p(ib), float(cutoff), count.ctypes.data):
            raise RuntimeError('cluster.count_within failed: %s' % lib.upside_hip_last_error().decode())
        return count
    finally:
        _done(A, B)


def kcenters(frames, k=None, cutoff=None, first=0, atoms=None, library=None):
    """farthest-point clustering (Gonzalez 1985).  Centre 0 is frame `first`; each round asks the device for every frame's distance to
    the one new centre (nearest), takes the elementwise minimum with the running distance (the lower centre number stays on equal bits)
    and makes the frame with the largest running distance the next centre (the lowest index on ties).  It stops at k centres, or when
    the largest distance is <= cutoff (at least one of the two must be given), or when every frame is a centre.  A centre is at
    distance exactly 0 of itself.  Returns (centers (K,) int64 frame indices, assignment (F,) int64 centre numbers, dist (F,))."""
    if k is None and cutoff is None:
        raise ValueError('cluster.kcenters: k or cutoff must be given')
    if k is not None and (int(k) != k or k < 1):
        raise ValueError('cluster.kcenters: k must be a whole number, at least 1')
    if cutoff is not None and not (np.ndim(cutoff) == 0 and np.isfinite(cutoff) and cutoff >= 0):
        raise ValueError('cluster.kcenters: cutoff must be one finite number, not negative')
    W = _Wrapped(frames, atoms, library, 'frames')
    try:
        F = W.f.n_frame
        if int(first) != first or not 0 <= first < F:
            raise ValueError('cluster.kcenters: first must lie in 0 .. %d' % (F - 1))
        centers = [int(first)]
        _, running = nearest(W.f, W.f, ib=[int(first)])
        running[int(first)] = 0.
        assignment = np.zeros(F, 'i8')
        while len(centers) < F and (k is None or len(centers) < int(k)):
            far = int(np.argmax(running))
            if cutoff is not None and running[far] <= cutoff:
                break
            if running[far] == 0.:      # (every frame left coincides with a centre)
                break
            _, d = nearest(W.f, W.f, ib=[far])
            d[far] = 0.
            closer = d < running
            assignment[closer] = len(centers)
            running = np.where(closer, d, running)
            centers.append(far)
        return np.array(centers, 'i8'), assignment, running
    finally:
        W.close()


def gromos(frames, cutoff, atoms=None, library=None):
    """the clustering of Daura et al. 1999.  count_within(all, all) gives every frame's neighbour count, itself included; then, until
    no frame is live: the live frame with the largest count (the lowest index on ties) becomes a centre, its members are the live
    frames with d <= cutoff of it (one rmsd_matrix row; the centre itself always), they are retired, and every live frame's count
    drops by count_within(live, members).  Two passes over the pair matrix in all, which is never stored.  Returns (centers (K,) int64
    frame indices, assignment (F,) int64 cluster numbers, sizes (K,) int64), the largest cluster first (found order among equals).
    A pair exactly at the cutoff may be counted and assigned differently by rounding (d2 <= cutoff^2 against sqrt(d2) <= cutoff)."""
    if not (np.ndim(cutoff) == 0 and np.isfinite(cutoff) and cutoff >= 0):
        raise ValueError('cluster.gromos: cutoff must be one finite number, not negative')
    W = _Wrapped(frames, atoms, library, 'frames')
    try:
        F = W.f.n_frame
        count = count_within(W.f, W.f, cutoff)
        live = np.ones(F, bool)
        found_assignment = np.full(F, -1, 'i8')
        centers, sizes = [], []
        while live.any():
            cand = np.flatnonzero(live)
            c = int(cand[np.argmax(count[cand])])
            row = rmsd_matrix(W.f, W.f, ia=[c], ib=cand)[0]
            members = cand[(row <= cutoff) | (cand == c)]
            found_assignment[members] = len(centers)
            centers.append(c); sizes.append(len(members))
            live[members] = False
            rest = np.flatnonzero(live)
            if len(rest):
                count[rest] -= count_within(W.f, W.f, cutoff, ia=rest, ib=members)
        return order_clusters(centers, found_assignment, sizes)
    finally:
        W.close()


def order_clusters(centers, assignment, sizes):
    """the clusters renumbered largest first (a stable sort: found order among equal sizes)"""
    centers = np.asarray(centers, 'i8'); sizes = np.asarray(sizes, 'i8'); assignment = np.asarray(assignment, 'i8')
    order = np.argsort(-sizes, kind='stable')
    number = np.empty(len(order), 'i8'); number[order] = np.arange(len(order))
    return centers[order], number[assignment], sizes[order]
