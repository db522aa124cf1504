#!/usr/bin/env python3
"""Cluster the frames of one or more output files by RMSD after optimal superposition, on the device (upside-md_amd/cluster.py):

    tools/cluster_frames.py out1.h5 [out2.h5 ...] --atoms ca|all (--cutoff A [--method gromos|kcenters] | --k N) --out clusters.npz

reads /output/pos of every file (frames x systems x atoms x 3; every system of a frame counts as a frame, in storage order) and
writes, with F frames and K clusters:
    centers (K, 2)   (file number, frame number within the file) of every cluster's centre
    center_frames (K,)  the same as positions among all frames
    assignment (F,)  the cluster of every frame        file_index (F,), frame_index (F,)  where every frame came from
    dist (F,)        the RMSD of every frame to its cluster's centre
    sizes (K,)       the members of every cluster
--cutoff with the method gromos (the default; Daura et al. 1999) gives the clusters largest first; with kcenters (Gonzalez 1985) it
adds centres until every frame lies within the cutoff of one; --k N gives kcenters with N centres.  --atoms ca takes every third
atom from the second (the C-alpha of an N, CA, C backbone), all takes every atom."""
import argparse
import os
import sys
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from __graft_entry__ import load_package  # noqa: E402


def read_frames(pkg, paths):
    pos, file_of, frame_of = [], [], []
    for k, path in enumerate(paths):
        with pkg.h5lite.open_file(path) as f:
            x = f.read('output/pos', 'f4')
        if x.ndim != 4 or x.shape[3] != 3:
            raise SystemExit('%s: /output/pos has shape %r, expected (frames, systems, atoms, 3)' % (path, x.shape))
        if pos and x.shape[2] != pos[0].shape[1]:
            raise SystemExit('%s: %d atoms per frame, the files before it have %d' % (path, x.shape[2], pos[0].shape[1]))
        x = x.reshape(-1, x.shape[2], 3)
        pos.append(x); file_of.append(np.full(len(x), k, 'i8')); frame_of.append(np.arange(len(x), dtype='i8'))
    return np.concatenate(pos), np.concatenate(file_of), np.concatenate(frame_of)


def cluster(pkg, pos, atoms, cutoff=None, method='gromos', k=None):
    """dict of the arrays the tool writes, but for file and frame"""
    cl = pkg.cluster
    with cl.Frames(pos, atoms=atoms) as fr:
        if k is not None or method == 'kcenters':
            centers, assignment, dist = cl.kcenters(fr, k=k, cutoff=cutoff)
            sizes = np.bincount(assignment, minlength=len(centers)).astype('i8')
        else:
            centers, assignment, sizes = cl.gromos(fr, cutoff)
            # one row per centre against its members, gathered into one call per centre
            dist = np.zeros(len(pos))
            for c, centre in enumerate(centers):
                members = np.flatnonzero(assignment == c)
                dist[members] = cl.rmsd_matrix(fr, fr, ia=[int(centre)], ib=members)[0]
                dist[centre] = 0.
    return dict(center_frames=centers, assignment=assignment, dist=dist, sizes=sizes)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('files', nargs='+')
    ap.add_argument('--atoms', choices=('ca', 'all'), required=True)
    ap.add_argument('--cutoff', type=float)
    ap.add_argument('--method', choices=('gromos', 'kcenters'), default='gromos')
    ap.add_argument('--k', type=int)
    ap.add_argument('--out', required=True)
    a = ap.parse_args(argv)
    if (a.cutoff is None) == (a.k is None):
        ap.error('give --cutoff or --k, one of the two')
    pkg = load_package()
    pos, file_of, frame_of = read_frames(pkg, a.files)
    atoms = np.arange(1, pos.shape[1], 3) if a.atoms == 'ca' else None
    r = cluster(pkg, pos, atoms, a.cutoff, a.method, a.k)
    cf = r['center_frames']
    np.savez(a.out, centers=np.stack([file_of[cf], frame_of[cf]], axis=1), file_index=file_of, frame_index=frame_of, **r)
    print('%d frames of %d files, %d clusters; the largest holds %d frames; largest distance to a centre %.3f' %
          (len(pos), len(a.files), len(cf), int(r['sizes'].max()), float(r['dist'].max())))


if __name__ == '__main__':
    main()
