"""`bt.phases` on the host: `Phase`, `Polyco` and `PolycoPhase` against vectors of the real
reference (tests/golden/phases_vectors.npz, recipe make_phases_golden.py), and the NumPy bin
function that defines the fold tables of a polynomial phase."""
import os

import numpy as np
import pytest

import baseband_tasks_amd as bt
from baseband_tasks_amd.fold_table import (phase_difference, phase_parts, piece_table, plan_pieces,
                                           polynomial_bins, unwrapped_bin)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_DIR = os.path.join(ROOT, 'tests', 'golden')
FILES = {'B1937': 'B1937_polyco.dat', 'B1957': 'B1957_polyco.dat'}

# Phase differences from the reference, in cycles.  The polynomial part is |p| <= 60 F0 span / 2
# cycles (B1937: 1.2e6, B1957: 5.6e6), one ulp of which is 2.3e-10 / 9.3e-10 cycle.  On top of
# that the reference takes the time from astropy's (jd1, jd2): the fraction of a day has a place
# of 2**-53 day = 9.6e-12 s, which is 6.2e-9 cycle at 642 Hz, and a time difference goes through
# a few such roundings; this package keeps whole seconds and the fraction apart (1e-13 s).
# Measured on the fixtures (largest |difference| over 252 times each): B1937 1.28e-8 cycle,
# B1957 6.6e-9 cycle -- two places of the reference's time.  Allowed: 4e-8 cycle, three times
# the larger (a different, equally valid order of the time arithmetic and the Horner steps).
# Frequencies: measured equal (0 relative difference), allowed 1e-12.
PHASE_TOL = 4e-8
FREQ_RTOL = 1e-12


@pytest.fixture(scope='module')
def golden():
    with np.load(os.path.join(GOLDEN_DIR, 'phases_vectors.npz'), allow_pickle=False) as g:
        yield {k: g[k] for k in g.files if not k.startswith('stream')}


def polyco(name):
    return bt.phases.Polyco(os.path.join(GOLDEN_DIR, FILES[name]))


def times(golden, name):
    sec, frac = golden[f'{name}/sec'], golden[f'{name}/frac']
    return bt.Time(int(sec[0]), float(frac[0])) + ((sec - sec[0]) + (frac - frac[0]))


def exact_times(golden, name):
    """The golden times one by one (whole seconds and fraction exactly as stored)."""
    return [bt.Time(int(s), float(f)) for s, f in zip(golden[f'{name}/sec'], golden[f'{name}/frac'])]


# -- Polyco ------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(FILES))
def test_polyco_table(golden, name):
    pc = polyco(name)
    assert len(pc) == 4
    np.testing.assert_array_equal(pc.mjd_mid, golden[f'{name}/mjd_mid'])
    np.testing.assert_array_equal(pc['f0'], golden[f'{name}/f0'])
    np.testing.assert_array_equal(pc['rphase'].int, golden[f'{name}/rphase_int'])
    np.testing.assert_allclose(pc['rphase'].frac, golden[f'{name}/rphase_frac'], rtol=0, atol=1e-15)
    np.testing.assert_array_equal(pc['coeff'], golden[f'{name}/coeff'])
    assert pc['mjd_mid'].dtype.names == ('int', 'frac')
    assert ('binphase' in pc.colnames) == (name == 'B1957')
    for key in ('psr', 'dm', 'span', 'freq', 'ncoeff', 'obs'):
        assert len(pc[key]) == 4


@pytest.mark.parametrize('name', sorted(FILES))
def test_polyco_phase_against_reference(golden, name):
    pc = polyco(name)
    t = exact_times(golden, name)
    got = [pc(x) for x in t]                                   # scalar times
    d = np.array([(p.int - i) + (p.frac - f) for p, i, f in
                  zip(got, golden[f'{name}/phase_int'], golden[f'{name}/phase_frac'])])
    print(f'{name}: largest phase difference from the reference {np.abs(d).max():.3e} cycle')
    assert np.abs(d).max() < PHASE_TOL
    assert all(isinstance(p, bt.phases.Phase) and p.isscalar and abs(p.frac) <= 0.5 for p in got)
    # array-valued time (offsets from the first in float64: 1e-11 s over the table's hours)
    ta = times(golden, name)
    pa = pc(ta)
    assert pa.shape == (len(t),)
    da = phase_difference(pa, bt.phases.Phase(golden[f'{name}/phase_int'], golden[f'{name}/phase_frac']))
    assert np.abs(da).max() < 1e-7
    np.testing.assert_array_equal(pc.searchclosest(ta), golden[f'{name}/index'])
    # the reference's own scalar calls
    for j, i in enumerate(golden[f'{name}/scalar_index']):
        assert abs((got[i].int - golden[f'{name}/scalar_int'][j])
                   + (got[i].frac - golden[f'{name}/scalar_frac'][j])) < PHASE_TOL


@pytest.mark.parametrize('name', sorted(FILES))
def test_polyco_rphase_forms_and_derivatives(golden, name):
    pc = polyco(name)
    t = exact_times(golden, name)
    for key, rphase in (('fraction', 'fraction'), ('ignore', 'ignore'), ('fixed', 0.25)):
        got = np.array([pc(x, rphase=rphase) for x in t])
        # (one float64 of ~1e6 cycles: its own rounding on top)
        assert np.abs(got - golden[f'{name}/{key}']).max() < PHASE_TOL + 2e-9, key
    freq = np.array([pc(x, deriv=1) for x in t])
    print(f'{name}: largest relative frequency difference '
          f'{np.abs(freq / golden[f"{name}/freq"] - 1).max():.3e}')
    np.testing.assert_allclose(freq, golden[f'{name}/freq'], rtol=FREQ_RTOL)
    fdot = np.array([pc(x, deriv=2, time_unit=bt.units.minute) for x in t])
    np.testing.assert_allclose(fdot, golden[f'{name}/fdot_per_min'], rtol=1e-6, atol=1e-9)
    # MJD floats (a microsecond of time: 1e-3 cycle)
    got = pc(golden[f'{name}/mjd'], rphase='fraction')
    assert np.abs(got - golden[f'{name}/mjd_phase']).max() < 1e-6 * pc['f0'][0] * 2
    # explicit index, and a time as index
    i = int(golden[f'{name}/index'][5])
    assert pc(t[5], index=i) == pc(t[5])
    assert pc(t[5], index=t[5]) == pc(t[5])


@pytest.mark.parametrize('name', sorted(FILES))
def test_polyco_polynomials(golden, name):
    pc = polyco(name)
    mid = pc.mjd_mid
    pol = pc.phasepol(1, rphase='fraction', t0=mid[1], time_unit=bt.units.s, convert=True)
    # (the constant is the phase at t0: to the tolerance of a phase)
    assert abs(pol.coef[0] - golden[f'{name}/phasepol_coef'][0]) < PHASE_TOL
    np.testing.assert_allclose(pol.coef[1:], golden[f'{name}/phasepol_coef'][1:], rtol=1e-9, atol=1e-30)
    fpol = pc.fpol(2, t0=mid[2], time_unit=bt.units.s, convert=True)
    np.testing.assert_allclose(fpol.coef, golden[f'{name}/fpol_coef'], rtol=1e-9, atol=1e-30)
    # polynomial(index) in minutes from TMID is what __call__ evaluates
    p = pc.polynomial(0, rphase='ignore')
    t = bt.Time.from_jd(2400000.5 + float(pc['mjd_mid']['int'][0]), float(pc['mjd_mid']['frac'][0])) + 60.
    assert abs(p(1.) - pc(t, index=0, rphase='ignore')) < 1e-6


@pytest.mark.parametrize('name', sorted(FILES))
def test_polyco_range(name):
    pc = polyco(name)
    lo = pc.mjd_mid[0] - pc['span'][0] / 2. / 1440.
    hi = pc.mjd_mid[-1] + pc['span'][-1] / 2. / 1440.
    with pytest.raises(ValueError):
        pc(lo - 1e-3)
    with pytest.raises(ValueError):
        pc(np.array([lo + 1e-3, hi + 1e-3]))
    pc(np.array([lo + 1e-3, hi - 1e-3]))
    with pytest.raises(ValueError):
        bt.phases.PolycoPhase(pc)(bt.Time('2001-01-01T00:00:00') + np.zeros(2))


@pytest.mark.parametrize('name,style', [('B1937', 'tempo1'), ('B1957', 'tempo2'), ('B1937', 'tempo2')])
def test_polyco_round_trip(tmp_path, name, style):
    pc = polyco(name)
    out = tmp_path / 'polyco.dat'
    pc.to_polyco(str(out), style=style)
    back = bt.phases.Polyco(str(out))
    assert back.colnames == pc.colnames and len(back) == len(pc)
    for key in pc.colnames:
        if key == 'date':                               # (tempo1 writes the month in capitals)
            assert [d.upper() for d in back[key]] == [d.upper() for d in pc[key]]
        elif key == 'rphase':
            assert np.all(back[key] == pc[key])
        else:
            np.testing.assert_array_equal(back[key], pc[key], err_msg=key)
    same_style = (name, style) in (('B1937', 'tempo1'), ('B1957', 'tempo2'))
    assert (back == pc) == same_style
    original = open(os.path.join(GOLDEN_DIR, FILES[name])).read().splitlines()
    written = out.read_text().splitlines()
    if same_style:                                      # (the style of the fixture)
        assert [line.split() for line in written] == [line.split() for line in original]


# -- Phase -------------------------------------------------------------------------------
def test_phase_arithmetic(golden):
    Phase = bt.phases.Phase
    a = Phase(golden['phase/a1'], golden['phase/a2'])
    b = Phase(golden['phase/b1'], golden['phase/b2'])
    results = dict(a=a, add=a + b, sub=a - b, neg=-a, mul=a * 3.7, div=a / 1.3, addf=a + 0.625, rsub=2.5 - b)
    for key, value in results.items():
        d = (value.int - golden[f'phase/{key}_int']) + (value.frac - golden[f'phase/{key}_frac'])
        # (two doubles carry ~1e11 cycles to 1e-16; products and quotients to 1e-5 ulp of the whole)
        assert np.abs(d).max() < (1e-15 if key not in ('mul', 'div') else 1e-10), key
        assert np.all(np.abs(value.frac) <= 0.5) and np.all(value.int == np.round(value.int)), key
    np.testing.assert_array_equal(a < b, golden['phase/less'])
    np.testing.assert_array_equal(a >= b, ~golden['phase/less'])
    assert np.all((a - a) == 0.) and np.all(a == a) and not np.any(a != a)
    assert a.shape == (50,) and a[3:5].shape == (2,) and a[7].isscalar
    np.testing.assert_array_equal(a.to_value('cycle'), a.int + a.frac)
    np.testing.assert_array_equal(a.cycle, a.int + a.frac)


def test_phase_strings(golden):
    Phase = bt.phases.Phase
    s = Phase.from_string(golden['phase/strings'])
    np.testing.assert_array_equal(s.int, golden['phase/strings_int'])
    np.testing.assert_allclose(s.frac, golden['phase/strings_frac'], rtol=0, atol=1e-16)
    one = Phase('162169181660.066162')
    assert one.int == 162169181660. and abs(one.frac - 0.066162) < 1e-16
    assert Phase(1.75).int == 2. and Phase(1.75).frac == -0.25
    assert Phase(1, 0.75) == Phase(2, -0.25)
    assert format(one, '20.6f') == ' 162169181660.066162'
    assert one.to_string(precision=6) == '162169181660.066162'
    with pytest.raises(ValueError):
        Phase.from_string(np.arange(3))
    with pytest.raises(ValueError):
        Phase('abc')


def test_phase_in_fold_table():
    Phase = bt.phases.Phase
    p = Phase(np.array([3., 4., 5e10]), np.array([0.25, -0.25, 0.5]))
    whole, frac = phase_parts(p)
    np.testing.assert_array_equal(whole, [3, 3, 50000000000])
    np.testing.assert_array_equal(frac, [0.25, 0.75, 0.5])
    np.testing.assert_array_equal(phase_difference(p, Phase(np.array([1., 1., 5e10]), 0.125)), [2.125, 2.625, 0.375])
    np.testing.assert_array_equal(unwrapped_bin(p, 8), [3 * 8 + 2, 3 * 8 + 6, 50000000000 * 8 + 4])


# -- the bin function --------------------------------------------------------------------
@pytest.mark.parametrize('name,start,rate,n_phase', [
    ('B1937', ('2018-05-06T22:20:00', 0.25), 1e6, 256),         # 6 samples per bin
    ('B1937', ('2018-05-06T22:57:20', 0.5), 1e5, 64),           # 2.4 samples per bin, over an entry change
    ('B1957', ('2014-06-09T23:59:50', 0.125), 2e5, 100),        # 3.2 samples per bin, over an entry change
    ('B1957', ('2014-06-09T22:00:00', 0.), 16e6, 256),          # 100 samples per bin
])
def test_bin_function_against_callable(name, start, rate, n_phase):
    """`polynomial_bins` on the pieces of `PolycoPhase.fold_pieces` against the bins of the
    callable's phases: equal except within rounding of a bin edge, at most 1e-6 of the samples."""
    pp = bt.phases.PolycoPhase(os.path.join(GOLDEN_DIR, FILES[name]))
    t_ref = bt.Time(start[0]) + start[1]
    n = 4_000_000
    pieces = pp.fold_pieces(t_ref, rate, 0, n)
    assert pieces[0][0] == 0 and pieces[-1][1] == n
    assert all(a[1] == b[0] for a, b in zip(pieces[:-1], pieces[1:]))
    if 'T22:57' in start[0] or 'T23:59' in start[0]:
        assert len(pieces) == 2
        # the cut is where the closest entry changes
        cut = pieces[1][0]
        idx = pp.polyco.searchclosest(t_ref + np.array([cut - 1, cut]) / rate)
        assert idx[1] == idx[0] + 1
    differ = 0
    for (a, b, coeff, dt0, step, ref_int, ref_frac) in pieces:
        m = np.arange(a, b, dtype=np.int64)
        k = pp.piece_bins(coeff, dt0, step, ref_int, ref_frac, m, n_phase)
        assert np.all(np.diff(k) >= 0)
        differ += np.count_nonzero(k != unwrapped_bin(pp(t_ref + m / rate), n_phase))
    print(f'{name} {rate:g} Hz, {n_phase} bins: {differ} of {n} samples differ')
    assert differ <= 1e-6 * n


def test_piece_table_is_the_per_sample_table():
    pp = bt.phases.PolycoPhase(os.path.join(GOLDEN_DIR, FILES['B1937']))
    t0, rate, n_phase = bt.Time('2018-05-06T22:57:29'), 1e4, 16
    edges = np.array([100, 30100, 60100, 200000])

    def row_pieces(r, lo, hi):
        return pp.fold_pieces(t0 + int(edges[r]) / rate, rate, lo - edges[r], hi - edges[r])
    c0, c1 = 20000, 150000
    r0, n_row, sp, rb, re, cnt = piece_table(edges, row_pieces, n_phase, c0, c1)
    assert (r0, n_row) == (0, 3) and cnt.sum() == c1 - c0
    # per sample
    slot = np.empty(c1 - c0, np.int64)
    for r in range(3):
        lo, hi = max(c0, edges[r]), min(c1, edges[r + 1])
        for (a, b, *piece) in row_pieces(r, lo, hi):
            slot[a + edges[r] - c0:b + edges[r] - c0] = r * n_phase + polynomial_bins(*piece, np.arange(a, b), n_phase) % n_phase
    np.testing.assert_array_equal(cnt, np.bincount(slot, minlength=3 * n_phase))
    for j in range(3 * n_phase):
        covered = np.concatenate([np.arange(b, e) for b, e in zip(rb[sp[j]:sp[j + 1]], re[sp[j]:sp[j + 1]])] or
                                 [np.zeros(0, np.int64)])
        np.testing.assert_array_equal(covered, np.flatnonzero(slot == j))


def test_piece_table_refuses_a_phase_that_steps_back():
    """Two linear pieces of 3 bins a sample, the second starting 6 bins back: the row's last bin is above its
    first, and its two ends are all that `plan_pieces` sees.  `piece_table` sees every sample and refuses, as
    the table kernel does (test_phase_runs_guard_gpu.py)."""
    n_phase, step = 8, 3. / 8.
    edges = np.array([0, 24])

    def row_pieces(back):
        ref_int = np.round(2. - back / 8.)
        both = [(0, 12, [0., 1.], 0., step, 2., 0.), (12, 24, [0., 1.], 0., step, ref_int, (2. - back / 8.) - ref_int)]
        return lambda r, lo, hi: [(max(a, lo), min(b, hi)) + tuple(piece) for a, b, *piece in both if a < hi and b > lo]
    k = np.concatenate([polynomial_bins(*piece, np.arange(a, b), n_phase) for a, b, *piece in row_pieces(6)(0, 0, 24)])
    np.testing.assert_array_equal(k, np.concatenate((16 + 3 * np.arange(12), 46 + 3 * np.arange(12))))
    assert plan_pieces(edges, row_pieces(6), n_phase, 0, 24)[2]['run_cap'] == 24           # (the plan passes it)
    for back in (6, 5, 4):                    # (onto bins the first piece visited, stepped over, and one bin back)
        with pytest.raises(ValueError, match='phase must increase with time'):
            piece_table(edges, row_pieces(back), n_phase, 0, 24)
    # standing still, or a later chunk that begins after the step, is no step back
    r0, n_row, sp, rb, re, cnt = piece_table(edges, row_pieces(3), n_phase, 0, 24)
    assert cnt.sum() == 24 and len(rb) == 23
    r0, n_row, sp, rb, re, cnt = piece_table(edges, row_pieces(6), n_phase, 12, 24)
    assert cnt.sum() == 12 and len(rb) == 12


def test_polyco_phase_offers_the_protocol():
    pp = bt.phases.PolycoPhase(os.path.join(GOLDEN_DIR, FILES['B1957']))
    assert callable(pp) and hasattr(pp, 'fold_pieces') and pp.piece_bins is polynomial_bins
    assert isinstance(pp.polyco, bt.phases.Polyco)
    assert bt.phases.PolycoPhase(pp.polyco).polyco is pp.polyco
    f = pp.apparent_spin_freq(bt.Time('2014-06-09T22:00:00') + np.arange(2.))
    assert np.all(np.abs(f - 622.122) < 0.1)
