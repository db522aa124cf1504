"""GPU tests of the torsional collective variables (kinds dihedral and dihedral_similarity of csrc/cv_device.h) and of the periodic
rule of the two biases built on them: every check runs in a child process with its own time limit
(tests/cv_dihedral_gpu_worker.py, which prints each figure before it asserts) against the float64 yardstick
tests/cv_dihedral_reference.py, itself pinned by tests/test_cv_dihedral_config.py.  Everything runs on trpcage20_7A (60 atoms); the
configuration files are written into the test's temporary directory.  Bounds: a value within parity_util.RTOL x max(|value|, 1), a
dihedral's difference taken on the circle; a bias energy within 1e-6 relative; a derivative within RTOL as relative RMS and 10 x RTOL
of its scale in the largest element; equalities between engine runs are bitwise."""
import os
import subprocess
import sys
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
WORKER = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'cv_dihedral_gpu_worker.py')


def run_check(which, tmp_path, timeout, env=None):
    try:
        r = subprocess.run([sys.executable, WORKER, which, str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=timeout,
                           env=dict(os.environ, **(env or {})))
    except subprocess.TimeoutExpired as err:      # a hang: nothing more is started
        pytest.exit('check %s did not finish in %d s:\n%s' % (which, timeout, (err.stdout or b'').decode()[-3000:]), returncode=3)
    out = r.stdout.decode()
    print(out)
    if r.returncode not in (0, 1):      # killed by a signal or aborted: nothing more is started on a device that may have faulted
        pytest.exit('check %s ended with status %d:\n%s' % (which, r.returncode, out[-3000:]), returncode=3)
    assert r.returncode == 0, out[-6000:]
    assert 'CHECK %s PASSED' % which in out, out[-2000:]
    return out


def test_values_match_the_float64_yardstick(tmp_path):
    """16 systems: the fixture plus seeded Gaussian noise growing from 0 to 3 Angstrom, the last with four atoms each in an exactly
    planar cis and trans arrangement; every phi and psi of backbone_dihedrals as its own dihedral, three omega torsions beside +-pi,
    dihedral_similarity over 1, 255, 256, 257 and 600 random quadruples, the helix content; every value within the bound, planar cis
    exactly 0 and trans exactly float32(pi); the phi / psi CVs of the noise-free system equal get_output('rama_coord')"""
    run_check('values', tmp_path, 300)


def test_rows_do_not_depend_on_the_batch(tmp_path):
    """identical positions at systems 0, 7 and the last of 64 systems give bit-identical rows; two runs are bit-identical"""
    run_check('batch', tmp_path, 300)


def test_restraint_matches_the_yardstick_across_the_cut(tmp_path):
    """the cv_restraint node alone on dihedrals (one with flat_width > 0, one inside its flat bottom, one with centre +3.0 and value
    -3.0), a dihedral_similarity over 257 quadruples, the helix content and an rg: energies and forces all together and each alone;
    restraint_values equals cvs() bitwise; collinear and coincident atoms give zero force and a finite energy"""
    run_check('restraint', tmp_path, 300)


def test_md_holds_a_torsion_at_its_window(tmp_path):
    """trpcage20 with its full potential, 8 systems at T = 0.8, psi of residue 10 with spring_const 50 and centres 0.9 pi (four
    systems) and -0.1 pi (four): after 200 rounds every value is closer on the circle to its own centre than to the other group's
    (the centres are pi apart: a margin of pi / 2); positions finite"""
    run_check('md', tmp_path, 300)


def test_metadynamics_matches_the_yardstick_across_the_cut(tmp_path):
    """the cv_metadynamics node alone, d = 2 over (phi, psi) of residue 10 placed beside +-pi and over (phi, rg): 1, 255, 256 and 257
    hills within +-2 sigma on both sides of the cut, energy and derivative; deposited centres are the bits of cvs(); well-tempered
    weights (kdT = 2) within 1e-6 of the yardstick's wrapped sum, with two hills written a period away from the walker"""
    run_check('metad', tmp_path, 300)


def test_captured_graph_replays_the_deposition(tmp_path):
    """12 rounds of (phi, psi) well-tempered metadynamics under UPSIDE_HIP_GRAPH=1 and =0: two runs of one setting bit-identical;
    hills, positions and momenta bit-identical between the settings"""
    res = {}
    for g in ('1', '0'):
        run_check('graph', tmp_path, 300, env={'UPSIDE_HIP_GRAPH': g})
        res[g] = np.load(str(tmp_path / ('graph%s.npz' % g)))
    same = dict((k, bool(np.array_equal(res['1'][k], res['0'][k]))) for k in ('pos', 'mom', 'centers', 'weights'))
    print('UPSIDE_HIP_GRAPH=1 against =0, bit-identical: %s' % same)
    assert all(same.values())


def test_recording_and_output_cv(tmp_path):
    """record_cvs over 40 rounds equals alternating run_rounds and cvs() bitwise; upside_hip on a file with a phi and a helix-content
    CV in /input/collective_variables writes /output/cv whose rows equal the yardstick on the stored frames within the bound"""
    run_check('record', tmp_path, 600)


def test_bad_definitions_are_refused_and_leave_the_previous_one_in_force(tmp_path):
    """a dihedral without exactly 4 atoms, a dihedral_similarity list that is no multiple of 4, a repeated atom in either kind,
    dihedral_ref missing (NULL and the old entry point with kind 5), not finite, of the wrong length or absent in a file; kinds 6 and 7
    still unknown: an error with the message, and cvs() still returns the earlier definition's values; a file without dihedral_ref
    loads as before; a ladder whose files differ in dihedral_ref is refused naming file, node and dataset"""
    run_check('refusals', tmp_path, 300)
