"""Generate tests/golden/phases_vectors.npz from the REAL reference's `Phase`, `Polyco`,
`PolycoPhase`, and its `Fold`, `PulseStack` and ``Integrate(phase=...)`` driven by a
`PolycoPhase`.

Run from this directory with a checkout of the reference (mhvk/baseband-tasks) on the
Python path and astropy installed, as for make_fold_golden.py:

    PYTHONPATH=<reference checkout> PYTHONDONTWRITEBYTECODE=1 \
        python3 -W ignore make_phases_golden.py

(the committed vectors: CPython 3.9, numpy 1.26, astropy 4.3.1).  The polyco files next to
this script are the reference's test data (baseband_tasks/tests/data).

Only data are written.  Times are stored as whole seconds since 1970-01-01 plus a fraction
(astropy's two-part 'unix' format keeps both), phases as their two parts.  For the fold
cases the recipe also imports this package (pure NumPy on this path) and counts the input
samples that the reference's per-sample bins and this package's `polynomial_bins` put in
different bins; the count is stored and must stay within 1e-6 of the samples.
"""
import json
import os
import sys

import numpy as np

for _name, _fn in (('asscalar', lambda a: np.asarray(a).item()),
                   ('alen', lambda a: len(np.asarray(a)))):
    if not hasattr(np, _name):
        setattr(np, _name, _fn)

from astropy import units as u            # noqa: E402
from astropy.time import Time             # noqa: E402

from baseband_tasks.generators import StreamGenerator                 # noqa: E402
from baseband_tasks.functions import Power                             # noqa: E402
from baseband_tasks.integration import Integrate, Fold, PulseStack     # noqa: E402
from baseband_tasks.phases import Phase, Polyco, PolycoPhase            # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
FILES = {'B1937': 'B1937_polyco.dat', 'B1957': 'B1957_polyco.dat'}
UNIX_MJD = 40587


def unix_time(sec, frac):
    return Time(np.asarray(sec, dtype=float), np.asarray(frac, dtype=float), format='unix', scale='utc',
                precision=9)


def polyco_cases(name, out):
    pc = Polyco(os.path.join(HERE, FILES[name]))
    rng = np.random.default_rng(sum(map(ord, name)))
    mid = pc['mjd_mid'].mjd
    half = pc['span'].to_value(u.day) / 2.
    lo, hi = (mid - half).min(), (mid + half).max()
    # random times inside the table, and times a millisecond to a second either side of the
    # instants where the closest entry changes
    mjd = list(rng.uniform(lo + 1e-4, hi - 1e-4, 240))
    for a, b in zip(mid[:-1], mid[1:]):
        for off in (-1., -1e-3, 1e-3, 1.):
            mjd.append((a + b) / 2. + off / 86400.)
    mjd = np.sort(np.array(mjd))
    seconds = (mjd - UNIX_MJD) * 86400.
    sec = np.floor(seconds)
    frac = np.round(rng.uniform(0., 1., len(sec)), 9)        # (any fraction: the whole second sets the place)
    t = unix_time(sec, frac)
    ph = pc(t)
    out[f'{name}/sec'] = sec.astype(np.int64)
    out[f'{name}/frac'] = frac
    out[f'{name}/phase_int'] = ph['int'].value
    out[f'{name}/phase_frac'] = ph['frac'].value
    out[f'{name}/index'] = pc.searchclosest(t)
    out[f'{name}/fraction'] = pc(t, rphase='fraction').value
    out[f'{name}/ignore'] = pc(t, rphase='ignore').value
    out[f'{name}/fixed'] = pc(t, rphase=0.25).value
    out[f'{name}/freq'] = pc(t, deriv=1).to_value(u.cycle / u.s)
    out[f'{name}/fdot_per_min'] = pc(t, deriv=2, time_unit=u.min).value
    # scalar times one at a time
    first = [pc(t[i]) for i in (0, 7, len(t) - 1)]
    out[f'{name}/scalar_index'] = np.array([0, 7, len(t) - 1])
    out[f'{name}/scalar_int'] = np.array([p['int'].value for p in first])
    out[f'{name}/scalar_frac'] = np.array([p['frac'].value for p in first])
    # MJD floats in
    out[f'{name}/mjd'] = mjd
    out[f'{name}/mjd_phase'] = pc(mjd, rphase='fraction').value
    # polynomials
    out[f'{name}/phasepol_coef'] = pc.phasepol(1, rphase='fraction', t0=mid[1], time_unit=u.s, convert=True).coef
    out[f'{name}/fpol_coef'] = pc.fpol(2, t0=mid[2], time_unit=u.s, convert=True).coef
    out[f'{name}/mjd_mid'] = mid
    out[f'{name}/f0'] = pc['f0'].value
    out[f'{name}/rphase_int'] = pc['rphase']['int'].value
    out[f'{name}/rphase_frac'] = pc['rphase']['frac'].value
    out[f'{name}/coeff'] = np.array(pc['coeff'])


def phase_cases(out):
    rng = np.random.default_rng(1957)
    a1 = np.round(rng.uniform(-1e11, 1e11, 50))
    a2 = rng.uniform(-3., 3., 50)
    b1 = np.round(rng.uniform(-1e11, 1e11, 50))
    b2 = rng.uniform(-3., 3., 50)
    a, b = Phase(a1, a2), Phase(b1, b2)
    out['phase/a1'], out['phase/a2'], out['phase/b1'], out['phase/b2'] = a1, a2, b1, b2
    for key, value in (('a', a), ('add', a + b), ('sub', a - b), ('neg', -a), ('mul', a * 3.7),
                       ('div', a / 1.3), ('addf', a + 0.625), ('rsub', 2.5 - b)):
        out[f'phase/{key}_int'] = value['int'].value
        out[f'phase/{key}_frac'] = value['frac'].value
    out['phase/less'] = np.asarray(a < b)
    strings = np.array(['162169181660.066162', '-0.5', '3.75', '1.25e3', '-1234.5625', '0.4999999999999', '7.0',
                        '2.5d0', '12.5e-1'])
    s = Phase.from_string(strings)
    out['phase/strings'] = strings
    out['phase/strings_int'] = s['int'].value
    out['phase/strings_frac'] = s['frac'].value


# ---------------------------------------------------------------------------------------------
FOLD_T0 = {'B1937': (1525645200, 0.25), 'B1957': (1402351200, 0.125)}     # 2018-05-06T22:20, 2014-06-09T22:00
RATE = 1.e6
N = 40000
CASES = [
    dict(kind='fold', psr='B1937', n_phase=256, step=0.01, start=0, average=True),
    dict(kind='fold', psr='B1937', n_phase=256, step=0.013, start=17, average=False),
    dict(kind='fold', psr='B1957', n_phase=256, step=None, start=0, average=False),
    dict(kind='fold', psr='B1957', n_phase=100, step=10000, start=0, average=True),
    dict(kind='pulsestack', psr='B1937', n_phase=32, start=0, average=True),
    dict(kind='integrate', psr='B1957', step=1. / 16, start=5, average=False),
]


def stream():
    rng = np.random.default_rng(20261017)
    return (rng.standard_normal((N, 2)) + 1j * rng.standard_normal((N, 2))).astype(np.complex64)


def reference_stream(psr, data):
    def frame(sh):
        return data[sh.tell():sh.tell() + sh.samples_per_frame]
    return StreamGenerator(frame, shape=data.shape, start_time=unix_time(*FOLD_T0[psr]),
                           sample_rate=RATE * u.Hz, samples_per_frame=1000, dtype=data.dtype,
                           polarization=np.array(['X', 'Y']))


def differing_bins(case, task):
    """Input samples of a fold case that the reference's phase puts in another bin than this
    package's `polynomial_bins` does (both per sample, the rows as `Fold` makes them)."""
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    import baseband_tasks_amd as bt
    from baseband_tasks_amd.phases import PolycoPhase as OurPhase
    ours = OurPhase(os.path.join(HERE, FILES[case['psr']]))
    theirs = PolycoPhase(os.path.join(HERE, FILES[case['psr']]))
    n_phase = case['n_phase']
    edges = task._get_offsets(np.arange(task.shape[0] + 1))
    differ = total = 0
    for r in range(task.shape[0]):
        a, b = int(edges[r]), int(edges[r + 1])
        m = np.arange(b - a)
        t_ref = unix_time(*FOLD_T0[case['psr']]) + (a / RATE) * u.s
        ph = theirs(t_ref + (m / RATE) * u.s)
        ref_bin = ((ph % (1. * u.cycle)) * n_phase).to_value(u.cycle).astype(int)
        our_ref = bt.Time(FOLD_T0[case['psr']][0], FOLD_T0[case['psr']][1]) + a / RATE
        k = np.concatenate([ours.piece_bins(p[2], p[3], p[4], p[5], p[6], np.arange(p[0], p[1]), n_phase)
                            for p in ours.fold_pieces(our_ref, RATE, 0, b - a)])
        differ += int(np.count_nonzero(k % n_phase != ref_bin))
        total += b - a
    return differ, total


def fold_cases(out):
    out['stream'] = stream()                    # (one seeded input for every case)
    for i, case in enumerate(CASES):
        psr = case['psr']
        sh = Power(reference_stream(psr, out['stream']))
        ph = PolycoPhase(os.path.join(HERE, FILES[psr]))
        meta = dict(case, t0=list(FOLD_T0[psr]), rate=RATE)
        if case['kind'] == 'fold':
            step = case['step']
            step = step if step is None or isinstance(step, int) else step * u.s
            task = Fold(sh, case['n_phase'], ph, step, start=case['start'], average=case['average'])
            differ, total = differing_bins(case, task)
            assert differ <= 1e-6 * total, (case, differ, total)
            meta.update(differing=differ, samples=total)
        elif case['kind'] == 'pulsestack':
            task = PulseStack(sh, case['n_phase'], ph, start=case['start'], average=case['average'])
        else:
            task = Integrate(sh, case['step'] * u.cycle, ph, start=case['start'], average=case['average'])
        result = task.read()
        meta.update(shape=list(task.shape))
        key = f'case{i:02d}'
        out[f'{key}/meta'] = np.array(json.dumps(meta))
        if result.dtype.names:
            out[f'{key}/data'] = result['data']
            out[f'{key}/count'] = result['count']
        else:
            out[f'{key}/data'] = result
        print(key, meta)


def main():
    out = {}
    for name in FILES:
        polyco_cases(name, out)
    phase_cases(out)
    fold_cases(out)
    np.savez_compressed(os.path.join(HERE, 'phases_vectors.npz'), **out)
    print('wrote', len(out), 'arrays')


if __name__ == '__main__':
    main()
