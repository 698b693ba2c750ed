"""Generate tests/golden/fold_vectors.npz from the REAL reference's `Fold`,
`PulseStack` and ``Integrate(phase=...)``.

Run from this directory with a checkout of the reference (mhvk/baseband-tasks)
on the Python path and astropy installed, as for make_golden.py:

    PYTHONPATH=<reference checkout> PYTHONDONTWRITEBYTECODE=1 \
        python3 -W ignore make_fold_golden.py

(the committed vectors: CPython 3.9, numpy 1.26, astropy 4.3.1).

Only data are written: the input streams, the outputs and, per case, its
parameters as JSON (phase parameters, never callables) and two margins: how far
every input sample's phase is from a bin edge (in bins) and how far every solved
or rounded offset is from a rounding tie (in samples).  Astropy's time
arithmetic and this package's differ in the last bits; the recipe refuses cases
whose margins are below 1e-6 bin / 2e-3 sample (the offset solve stops at
1e-3 sample).  (The fake pulsar of the
reference's tests has its phase zero on a sample, so half its samples sit on bin
edges; here its phase is shifted by 0.0013 cycle.)
"""
import json
import os

import numpy as np

for _name, _fn in (('asscalar', lambda a: np.asarray(a).item()),
                   ('alen', lambda a: len(np.asarray(a)))):
    if not hasattr(np, _name):
        setattr(np, _name, _fn)

from astropy import units as u            # noqa: E402
from astropy.time import Time             # noqa: E402

from baseband_tasks.generators import StreamGenerator                 # noqa: E402
from baseband_tasks.integration import Integrate, Fold, PulseStack     # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
T0 = '2010-11-12T13:14:15'
RATE = 10000.                            # Hz
N = 16000


def streams():
    rng = np.random.default_rng(20261016)
    pulsar = np.repeat(np.where(np.arange(N) % 125 == 0, 10., 0.125)[:, None], 2, axis=1).astype(np.float32)
    real = rng.standard_normal((N, 3)).astype(np.float32) + 1.5
    cplx = (rng.standard_normal((N, 3)) + 1j * rng.standard_normal((N, 3))).astype(np.complex64)
    return {'pulsar': pulsar, 'real': real, 'complex': cplx}


def reference_stream(data):
    def frame(sh):
        return data[sh.tell():sh.tell() + sh.samples_per_frame]
    return StreamGenerator(frame, shape=data.shape, start_time=Time(T0, precision=9),
                           sample_rate=RATE * u.Hz, samples_per_frame=200, dtype=data.dtype)


def reference_phase(p):
    t0 = Time(T0, precision=9)

    def phase(t):
        dt = (t - t0).to_value(u.s)
        return u.cycle * (p['phi0'] + p['f0'] * dt + 0.5 * p['f1'] * dt * dt)
    return phase


def cycles(p, dt):
    return p['phi0'] + p['f0'] * dt + 0.5 * p['f1'] * dt * dt


def step_value(spec):
    return None if spec is None else (spec if isinstance(spec, int) else spec * u.s)


def start_value(spec):
    if isinstance(spec, dict):
        return Time(T0, precision=9) + spec['time'] * u.s
    return spec


PULSAR = dict(phi0=0.0013, f0=80., f1=0.)         # (0.065 bin off the edges)
SPIN = dict(phi0=0.2137, f0=73.31, f1=-1.9)
CASES = []
for step in (0.01, 0.03, 0.026, 1. / 3., 270, None):
    for start in (0, {'time': 0.0313}):
        for average in (True, False):
            CASES.append(dict(kind='fold', stream='pulsar', n_phase=50, phase=PULSAR, step=step, start=start,
                              average=average))
for n_phase in (7, 37, 1024):
    CASES.append(dict(kind='fold', stream='real', n_phase=n_phase, phase=SPIN, step=0.1, start=37,
                      average=False))
CASES.append(dict(kind='fold', stream='complex', n_phase=37, phase=SPIN, step=0.26, start=0, average=True))
CASES.append(dict(kind='fold', stream='real', n_phase=50, phase=SPIN, step=None, start={'time': 0.2}, average=False))
CASES.append(dict(kind='integrate', stream='pulsar', phase=PULSAR, step=1. / 25, start=0, average=True))
CASES.append(dict(kind='integrate', stream='real', phase=dict(SPIN, f1=-2.3), step=1. / 3, start=0, average=False))
CASES.append(dict(kind='pulsestack', stream='pulsar', n_phase=25, phase=PULSAR, start=124, average=True))
CASES.append(dict(kind='pulsestack', stream='pulsar', n_phase=25, phase=PULSAR, start=0, average=True,
                  slice_input=[-360, -10]))
CASES.append(dict(kind='pulsestack', stream='pulsar', n_phase=25, phase=PULSAR, start=124, average=True,
                  slice_output=[10, 100]))
CASES.append(dict(kind='integrate_stack', stream='pulsar', n_phase=25, phase=PULSAR, start=0, average=True,
                  n=3))


def build(case, data):
    sh = reference_stream(data)
    if 'slice_input' in case:
        sh = sh[case['slice_input'][0]:case['slice_input'][1]]
    ph = reference_phase(case['phase'])
    start = start_value(case['start'])
    if case['kind'] == 'fold':
        return Fold(sh, case['n_phase'], ph, step_value(case['step']), start=start, average=case['average'])
    if case['kind'] == 'integrate':
        return Integrate(sh, case['step'] * u.cycle, ph, start=start, average=case['average'])
    ps = PulseStack(sh, case['n_phase'], ph, start=start, average=case['average'])
    if 'slice_output' in case:
        return ps[case['slice_output'][0]:case['slice_output'][1]]
    if case['kind'] == 'integrate_stack':
        return Integrate(ps, case['n'])
    return ps


def margins(case, task, data):
    """(bin margin, offset margin) computed in float64 from the analytic phase."""
    p = case['phase']
    first = case['slice_input'][0] % N if 'slice_input' in case else 0
    n = np.arange(first, N if 'slice_input' not in case else case['slice_input'][1] % N)
    dt = n / RATE
    off_margin = 0.5
    if case['kind'] == 'fold':
        x = cycles(p, dt) * case['n_phase']
        bin_margin = np.abs(x - np.round(x)).min()
        inner = task
        o = np.arange(task.shape[0] + 1) / inner._mean_offset_size + inner._ih_start
        off_margin = np.abs(np.abs(o - np.floor(o)) - 0.5).min()
    else:
        n_phase = case.get('n_phase')
        step = 1. / n_phase if n_phase else case['step']
        t_start = (start_value(case['start']) - Time(T0, precision=9)).to_value(u.s) \
            if isinstance(case['start'], dict) else (first + case['start']) / RATE
        rel = (cycles(p, dt) - cycles(p, t_start)) / step
        bin_margin = 0.5                  # (no per-sample bins: the offsets decide)
        # offsets where the relative phase crosses k * step
        k = np.arange(int(rel.max()) + 1)
        crossing = np.interp(k, rel, n)
        off_margin = np.abs(np.abs(crossing - np.floor(crossing)) - 0.5).min()
    return float(bin_margin), float(off_margin)


def main():
    data = streams()
    out = {f'stream/{k}': v for k, v in data.items()}
    for i, case in enumerate(CASES):
        task = build(case, data[case['stream']])
        result = task.read()
        bm, om = margins(case, task if case['kind'] == 'fold' else None, data[case['stream']])
        assert bm >= 1e-6 and om >= 2e-3, (i, case, bm, om)
        key = f'case{i:02d}'
        meta = dict(case, shape=list(task.shape), bin_margin=bm, offset_margin=om,
                    start_time=task.start_time.isot, stop_time=task.stop_time.isot,
                    sample_rate=float(task.sample_rate.value))
        out[f'{key}/meta'] = np.array(json.dumps(meta))
        if result.dtype.names:
            out[f'{key}/data'] = result['data']
            out[f'{key}/count'] = result['count']
        else:
            out[f'{key}/data'] = result
    np.savez_compressed(os.path.join(HERE, 'fold_vectors.npz'), **out)
    print('wrote', len(CASES), 'cases')


if __name__ == '__main__':
    main()
