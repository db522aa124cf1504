"""The two float -> fixed-point conversions of the pair passes' gradient accumulators, restated for the host (fixed_point_host.cpp, a
stand-alone program compiled here) and compared with exact integer arithmetic: what each form can hold and how finely, at the
edges of its range.  No GPU."""
import math
import os
import struct
import subprocess
from fractions import Fraction
import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope='module')
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('fixed_point') / 'fixed_point_host')
    subprocess.run(['g++', '-O1', '-std=c++11', '-ffp-contract=off', '-Wall', '-o', exe, os.path.join(HERE, 'fixed_point_host.cpp')], check=True)

    def run(mode, values):
        bits = ['%08x' % struct.unpack('<I', struct.pack('<f', v))[0] for v in values]
        out = subprocess.run([exe, mode] + bits, check=True, stdout=subprocess.PIPE).stdout.decode().split('\n')
        return [tuple(int(t) for t in line.split()) for line in out if line]
    return run


def f32(x):
    return float(np.float32(x))


def below(x):
    return float(np.nextafter(np.float32(x), np.float32(0)))


def round_half_even(q):
    f = math.floor(q)
    r = q - f
    return f + (1 if r > Fraction(1, 2) or (r == Fraction(1, 2) and f % 2) else 0)


def trunc(q):
    return math.floor(q) if q >= 0 else -math.floor(-q)


def test_to_fixed32_range_and_resolution(program):
    """-2^31 <= v < 2^31 in counts of 2^-32: off by less than 2^-31, exact for every multiple of 2^-31 -- up to the largest float below
    2^31 and at -2^31 itself; from 2^31 on the high word saturates (the result stays just below 2^31: no wrap to the other sign)"""
    rng = np.random.RandomState(5)
    vals = [0., 0.5, -0.5, 1.5, 2.5, -1.5, 0.49999997, 2. ** -31, -2. ** -31, 2. ** -32, 3 * 2. ** -33, 511.99997, 512., -600.25, 1e-30,
            below(2. ** 31), -below(2. ** 31), -2. ** 31, 2. ** 30 + 64., 8388607.5, -8388608.5, 1e9 + 64]
    vals += [f32(s * 2. ** e * (1. + rng.rand())) for e in range(-36, 31) for s in (1., -1.)]
    vals = [f32(v) for v in vals]
    got = program('32', vals)
    for v, (q,) in zip(vals, got):
        x = Fraction(v)
        h = round_half_even(x)
        want = h * 2 ** 32 + 2 * trunc((x - h) * 2 ** 31)
        assert q == want, (v, q, want)
        assert abs(Fraction(q) - x * 2 ** 32) < 2, (v, q)
        if (x * 2 ** 31).denominator == 1:
            assert Fraction(q) == x * 2 ** 32, (v, q)
    # beyond the range: saturation of the 32-bit conversion of the high word, documented beside to_fixed32
    (top,), (over,), (under,), (nan,) = program('32', [2. ** 31, 1e20, -1e20, float('nan')])
    assert top == over == (2 ** 31 - 1) * 2 ** 32 and under == -2 ** 63 and nan == 0


def test_fixed22_wide_path(program):
    """a scaled contribution vs = v * 2^22: floor(vs + 1/2) below 2^30 (the 32-bit conversion, off by at most half a count = 2^-23 in
    v), the exact integer from 2^30 to below 2^46 (|v| < 2^24), the error flag from 2^46 on and for NaN and infinity -- never a clean zero"""
    rng = np.random.RandomState(6)
    vals = [0., 0.5, -0.5, 1.5, 2.5, -2.5, 0.49999997, -0.49999997, 8388607.5, -8388607.5, below(2. ** 30), 2. ** 30, -2. ** 30, 600. * 2 ** 22, 512. * 2 ** 22,
            below(2. ** 31), 2. ** 31, -2. ** 31, 2. ** 31 + 256, 2. ** 40 + 2 ** 20, below(2. ** 46), -below(2. ** 46)]
    vals += [f32(s * 2. ** e * (1. + rng.rand())) for e in range(-4, 46) for s in (1., -1.)]
    vals = [f32(v) for v in vals]
    for v, (q, flag) in zip(vals, program('22', vals)):
        x = Fraction(v)
        want = math.floor(x + Fraction(1, 2)) if abs(x) < 2 ** 30 else int(x)
        assert flag == 0 and q == want, (v, q, flag, want)
        assert abs(Fraction(q) - x) <= Fraction(1, 2)
    for v in (2. ** 46, -2. ** 46, 1e30, float('inf'), -float('inf'), float('nan')):
        assert program('22', [v]) == [(0, 1)], v


def test_trip_check_never_lets_a_large_value_into_the_32_bit_conversion(program):
    """one comparison serves the two pairs of a trip: wherever it chooses the 32-bit conversions, every value is finite and below 2^30"""
    rng = np.random.RandomState(7)
    small = [f32(x) for x in rng.uniform(-1e6, 1e6, 12)]
    assert program('sq', small) == [(1,)]
    assert program('sq', [f32(50. * 2 ** 22)] * 14) == [(1,)]             # the largest contributions of the shipped force field
    for bad in (2. ** 30, -2. ** 30, below(2. ** 31), 2. ** 31, 3e38, -3e38, float('inf'), -float('inf'), float('nan')):
        for at in range(12):
            v = list(small); v[at] = f32(bad)
            assert program('sq', v) == [(0,)], (bad, at)
    for trial in range(200):
        v = [f32(s) for s in rng.uniform(-1, 1, 12) * 2. ** rng.randint(20, 33)]
        if program('sq', v)[0][0]:
            assert all(abs(s) < 2. ** 30 for s in v), v
