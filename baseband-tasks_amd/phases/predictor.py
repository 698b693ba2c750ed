"""Tempo polyco tables: read, evaluate, write (the reference's
`baseband_tasks.phases.Polyco`, on NumPy arrays instead of an astropy table).

A polyco file holds one entry per time span::

    line 1: pulsar name, date (dd-mmm-yy), UTC (hhmmss.ss), TMID (MJD), dispersion measure,
            Doppler shift (1e-4), log10 of the fit rms (periods)
    line 2: reference phase RPHASE, rotation frequency F0 (Hz), observatory, span (minutes),
            number of coefficients, observing frequency (MHz) [, binary phase, orbital
            frequency (1/day)]
    then the coefficients, three per line (Fortran ``D`` exponents in tempo1 files)

and predicts, for ``DT = (T - TMID) * 1440`` minutes::

    PHASE = RPHASE + DT*60*F0 + COEFF(1) + DT*COEFF(2) + DT^2*COEFF(3) + ...
    FREQ  = F0 + (1/60) * (COEFF(2) + 2*DT*COEFF(3) + 3*DT^2*COEFF(4) + ...)

(http://tempo.sourceforge.net/ref_man_sections/tz-polyco.txt).  TMID and RPHASE are kept
as two doubles each, (whole part, fraction), as read from the digits of the file.
"""
import datetime as _dt
import operator
import os

import numpy as np
from numpy.polynomial import Polynomial

from .. import units as u
from ..units import Time
from .phase import Phase, _parse_decimal

__all__ = ['Polyco']

_TWO_PART = np.dtype([('int', np.int64), ('frac', np.float64)])
_MJD_UNIX = 40587                              # MJD of 1970-01-01
_MINUTE = 60.
_DAY = 86400.

# header fields in file order: (name, line, kind); formats for writing are in `to_polyco`
_FIELDS = (('psr', str), ('date', str), ('utc_mid', float), ('mjd_mid', 'two'), ('dm', float),
           ('vbyc_earth', float), ('lgrms', float), ('rphase', 'two'), ('f0', float), ('obs', str),
           ('span', float), ('ncoeff', int), ('freq', float), ('binphase', float), ('forb', float))
_LINE1 = 7                                     # fields on the first header line


def _two_part(text):
    whole, frac = _parse_decimal(text)
    return int(whole), float(frac)


def _mjd_parts(time):
    """`Time` (scalar or array) or MJD float(s) -> (whole MJD as int64, seconds of the day,
    rest in seconds): for a `Time` the seconds of the day are whole and the rest is its
    fraction of a second, so that differences keep ~1e-13 s."""
    if u.is_time(time):
        if not isinstance(time, Time):
            time = Time(time)
        day, rest = np.divmod(time.sec, 86400)
        return np.asarray(day, np.int64) + _MJD_UNIX, np.asarray(rest, dtype=float), np.asarray(time.frac, float)
    mjd = np.asarray(time, dtype=float)
    whole = np.floor(mjd)
    return whole.astype(np.int64), (mjd - whole) * _DAY, np.zeros((), float)


def _minutes(parts, mid_int, mid_frac):
    whole, sod, rest = parts
    return ((whole - mid_int) * 1440. + (sod / _MINUTE - mid_frac * 1440.)) + rest / _MINUTE


class Polyco:
    """Polyco table.

    Parameters
    ----------
    data : str, path, or dict of columns
        File in tempo1 / tempo2 polyco format, or the columns of another `Polyco`.

    Columns (``polyco['f0']``, ``polyco.colnames``): ``psr``, ``date``, ``utc_mid``,
    ``mjd_mid`` (structured: ``'int'``, ``'frac'``), ``dm``, ``vbyc_earth``, ``lgrms``,
    ``rphase`` (a `Phase`), ``f0`` (Hz), ``obs``, ``span`` (minutes), ``ncoeff``, ``freq``
    (MHz), ``coeff`` (one row of coefficients per entry) and, if the file has them,
    ``binphase`` and ``forb``.  ``polyco[i]`` / ``polyco[i:j]`` select entries.

    Calling it predicts phases (see `__call__`).
    """

    def __init__(self, data):
        if isinstance(data, (str, bytes, os.PathLike)):
            data = _read(data)
        elif isinstance(data, Polyco):
            data = data._columns
        self._columns = {k: (v.copy() if hasattr(v, 'copy') else v) for k, v in data.items()}
        n = len(self._columns['f0'])
        if any(len(v) != n for v in self._columns.values()):
            raise ValueError("polyco columns differ in length")

    # -- table access -----------------------------------------------------------------
    @property
    def colnames(self):
        return list(self._columns)

    def keys(self):
        return list(self._columns)

    def __len__(self):
        return len(self._columns['f0'])

    def __getitem__(self, item):
        if isinstance(item, str):
            return self._columns[item]
        if isinstance(item, (int, np.integer)):
            item = slice(item, item + 1 if item != -1 else None)
        return Polyco({k: v[item] for k, v in self._columns.items()})

    def __repr__(self):
        if not len(self):
            return "<Polyco: empty>"
        return (f"<Polyco {self['psr'][0]}: {len(self)} entries, MJD "
                f"{self.mjd_mid[0]:.5f} .. {self.mjd_mid[-1]:.5f}>")

    @property
    def mjd_mid(self):
        """TMID as one float64 MJD per entry (about a microsecond; the two parts are in
        ``polyco['mjd_mid']``)."""
        c = self._columns['mjd_mid']
        return c['int'] + c['frac']

    def __eq__(self, other):
        if not isinstance(other, Polyco) or self.colnames != other.colnames or len(self) != len(other):
            return False
        for k, v in self._columns.items():
            w = other._columns[k]
            same = (np.all(v == w) if isinstance(v, Phase) else np.array_equal(v, w))
            if not same:
                return False
        return True

    __hash__ = None

    # -- evaluation -------------------------------------------------------------------
    def searchclosest(self, mjd):
        """Index of the entry whose TMID is closest to the (array of) `Time` / MJD."""
        if u.is_time(mjd):
            whole, sod, rest = _mjd_parts(mjd)
            mjd = whole + (sod + rest) / _DAY
        mjd = np.asarray(mjd, dtype=float)
        mid = self.mjd_mid
        if len(mid) == 1:
            return np.zeros(mjd.shape, np.int64)[()]
        i = np.clip(np.searchsorted(mid, mjd), 1, len(mid) - 1)
        return i - (mjd - mid[i - 1] < mid[i] - mjd)

    def minutes_from_mid(self, time, index):
        """``DT`` of the prediction formula: minutes from the TMID of entry ``index``
        (an index per time, or one for all), from the two parts of both."""
        mid = self._columns['mjd_mid'][index]
        return _minutes(_mjd_parts(time), mid['int'], mid['frac'])

    def _check_range(self, time):
        parts = _mjd_parts(time)
        mid, half = self._columns['mjd_mid'], self._columns['span'] / 2.
        first, last = np.argmin(self.mjd_mid - half / 1440.), np.argmax(self.mjd_mid + half / 1440.)
        before = _minutes(parts, mid['int'][first], mid['frac'][first]) < -half[first]
        after = _minutes(parts, mid['int'][last], mid['frac'][last]) > half[last]
        if np.any(before | after):
            raise ValueError('(some) MJD outside of polyco range')

    def coefficients(self, index, rphase='ignore'):
        """Coefficients of the phase polynomial of entry ``index`` in minutes from its TMID:
        ``COEFF`` with ``60 F0`` added to the linear term, and the phase zero point
        ``rphase`` (as for `polynomial`) to the constant."""
        c = np.array(self._columns['coeff'][index][:int(self._columns['ncoeff'][index])], dtype=float)
        if len(c) < 2:
            c = np.concatenate((c, np.zeros(2 - len(c))))
        c[1] += self._columns['f0'][index] * _MINUTE
        if rphase is None:
            c[0] += self._columns['rphase'][index].cycle
        elif isinstance(rphase, str):
            if rphase == 'fraction':
                c[0] += self._columns['rphase'].frac[index] % 1
            elif rphase != 'ignore':
                raise ValueError("rphase must be None, 'fraction', 'ignore' or a number")
        else:
            c[0] = rphase
        return c

    def __call__(self, time, index=None, rphase=None, deriv=0, time_unit=u.s):
        """Predicted phase, or frequency and its derivatives.

        Parameters
        ----------
        time : `~baseband_tasks_amd.units.Time` (scalar or array-valued) or MJD float(s)
            (a float MJD is good to about a microsecond only).
        index : int (array), None, MJD float or `Time`
            Entries to use; None: the closest to each time (after a check that the times
            are inside the table; `ValueError` if not); a time: the closest to that.
        rphase : None, 'fraction', 'ignore' or float
            Phase zero point: the stored RPHASE (None; the result is then a `Phase`, which
            keeps the ~1e11 cycles and the fraction apart), RPHASE modulo one, nothing, or
            the number given.
        deriv : int
            0: phase; 1: frequency; 2: its derivative; ...
        time_unit : float
            Seconds per unit of time of a derivative (default 1: cycles / s**deriv).

        Returns
        -------
        `Phase` for ``deriv=0, rphase=None``, otherwise float64 cycles (/ time_unit**deriv).
        """
        scalar_in = np.ndim(_mjd_parts(time)[0]) == 0
        try:
            index = operator.index(index)
        except TypeError:
            if index is None:
                self._check_range(time)
                index = self.searchclosest(time)
            elif u.is_time(index) or np.asarray(index).dtype.kind == 'f':
                index = self.searchclosest(index)
            else:
                index = np.asarray(index, dtype=np.int64)
        dt = np.asarray(self.minutes_from_mid(time, index), dtype=float)
        do_phase = deriv == 0 and rphase is None
        if do_phase:
            rphase = 'ignore'
        index_a = np.broadcast_to(np.asarray(index), dt.shape)
        result = np.zeros(dt.shape)
        for j in np.unique(index_a):
            sel = index_a == j
            c = self.coefficients(int(j), rphase)
            for _ in range(deriv):
                c = c[1:] * np.arange(1, len(c))
            x = dt[sel]
            p = np.full(x.shape, c[-1] if len(c) else 0.)
            for cj in c[-2::-1]:
                p = p * x + cj
            result[sel] = p
        if deriv:
            result *= (u.to_seconds(time_unit) / _MINUTE) ** deriv
        if scalar_in:
            result = result[()]
        if do_phase:
            return self._columns['rphase'][index_a if not scalar_in else int(index_a)] + result
        return result

    def polynomial(self, index, rphase=None, deriv=0, t0=None, time_unit=u.minute, out_unit=None,
                   convert=False):
        """`numpy.polynomial.Polynomial` of entry ``index`` (an index, or an MJD / `Time` for
        the closest entry).

        Its argument is in ``time_unit`` (seconds per unit; default minutes) counted from
        ``t0`` (MJD or `Time`; default: the entry's TMID), its value in cycles, or for
        ``deriv > 0`` in cycles / out_unit**deriv (default: ``time_unit``).  ``convert``
        gives it the unit domain.
        """
        out_unit = time_unit if out_unit is None else out_unit
        try:
            index = operator.index(index)
        except TypeError:
            index = int(self.searchclosest(index))
        window = np.array([-1., 1.]) * self._columns['span'][index] / 2.
        if deriv == 0:
            pol = Polynomial(self.coefficients(index, rphase), window, window)
        else:
            pol = Polynomial(self.coefficients(index, 'ignore'), window, window).deriv(deriv)
            pol.coef /= (_MINUTE / u.to_seconds(out_unit)) ** deriv
        if t0 is not None:
            dt = float(self.minutes_from_mid(t0, index))
            pol.domain = (window - dt) * _MINUTE / u.to_seconds(time_unit)
        return pol.convert() if convert else pol

    def phasepol(self, index, rphase=None, t0=0., time_unit=u.day, convert=False):
        """Phase polynomial in ``time_unit`` (default days) from the MJD ``t0``."""
        return self.polynomial(index, rphase, t0=t0, time_unit=time_unit, convert=convert)

    def fpol(self, index, t0=0., time_unit=u.day, convert=False):
        """Frequency polynomial (Hz) in ``time_unit`` (default days) from the MJD ``t0``."""
        return self.polynomial(index, deriv=1, t0=t0, time_unit=time_unit, out_unit=u.s, convert=convert)

    # -- writing ----------------------------------------------------------------------
    def to_polyco(self, name='polyco.dat', style='tempo2'):
        """Write the table as a polyco file in the style of 'tempo1' (upper-case month,
        ``0.dddD+ee`` coefficients) or 'tempo2'."""
        if style not in ('tempo1', 'tempo2'):
            raise ValueError("style must be 'tempo1' or 'tempo2'")
        col = self._columns
        with open(name, 'w') as fh:
            for i in range(len(self)):
                mjd_int, mjd_frac = int(col['mjd_mid']['int'][i]), float(col['mjd_mid']['frac'][i])
                date = (_dt.date(1858, 11, 17) + _dt.timedelta(days=mjd_int)).strftime('%d-%b-%y')
                if style == 'tempo1':
                    date = date.upper()
                if date[0] == '0':
                    date = ' ' + date[1:]
                centi = int(round(mjd_frac * _DAY * 100.))
                hh, rest = divmod(centi, 360000)
                mm, ss = divmod(rest, 6000)
                utc = hh * 10000. + mm * 100. + ss / 100.
                mid = Phase._from_parts(float(mjd_int), mjd_frac)
                line1 = (f"{col['psr'][i]:<10s}{date:>10s}{utc:11.2f}{mid:20.11f}{col['dm'][i]:21.6f}"
                         f"{col['vbyc_earth'][i]:7.3f}{col['lgrms'][i]:7.3f}")
                line2 = (f"{col['rphase'][i]:20.6f}{col['f0'][i]:18.12f}{col['obs'][i]:>5s}"
                         f"{col['span'][i]:5.0f}{int(col['ncoeff'][i]):5d}{col['freq'][i]:10.3f}")
                if 'binphase' in col:
                    line2 += f"{col['binphase'][i]:7.4f}"
                if 'forb' in col:
                    line2 += f"{col['forb'][i]:9.4f}"
                fh.write(line1 + '\n' + line2 + '\n')
                coeff = col['coeff'][i][:int(col['ncoeff'][i])]
                fmt = _fortran if style == 'tempo1' else '{:24.17e}'.format
                for j in range(0, len(coeff), 3):
                    fh.write(' ' + ' '.join(fmt(c) for c in coeff[j:j + 3]) + '\n')


def _fortran(x):
    """0.ddddddddddddddddD+ee: 17 significant digits with the point before the first."""
    mantissa, _, exponent = format(x, '.16e').partition('e')
    sign = '-' if mantissa.startswith('-') else ' '
    digits = mantissa.lstrip('-').replace('.', '')
    return f"{sign}0.{digits}D{int(exponent) + 1:+03d}"


def _read(name):
    entries = []
    with open(name, 'r') as fh:
        lines = [line for line in fh.read().splitlines()]
    pos = 0
    while pos < len(lines):
        if not lines[pos].strip():
            pos += 1
            continue
        first, second = lines[pos].split(), lines[pos + 1].split()
        pos += 2
        if len(first) != _LINE1:
            raise ValueError(f"{name}: header line of {len(first)} fields, expected {_LINE1}")
        entry = {}
        for (key, kind), text in zip(_FIELDS, first + second):
            entry[key] = _two_part(text) if kind == 'two' else kind(text)
        coeff = []
        while len(coeff) < entry['ncoeff']:
            coeff += lines[pos].split()
            pos += 1
        entry['coeff'] = [float(c.lower().replace('d', 'e')) for c in coeff]
        entries.append(entry)
    if not entries:
        raise ValueError(f"{name}: no polyco entries")
    keys = list(entries[0])
    if any(list(e) != keys for e in entries):
        raise ValueError(f"{name}: entries differ in their header fields")
    columns = {}
    width = max(len(e['coeff']) for e in entries)
    for key in keys:
        values = [e[key] for e in entries]
        if key == 'mjd_mid':
            columns[key] = np.array(values, dtype=_TWO_PART)
        elif key == 'rphase':
            columns[key] = Phase._from_parts([float(v[0]) for v in values], [v[1] for v in values])
            columns[key] = Phase(columns[key].int, columns[key].frac)     # (fraction into [-0.5, 0.5])
        elif key == 'coeff':
            columns[key] = np.array([v + [0.] * (width - len(v)) for v in values], dtype=float)
        else:
            columns[key] = np.array(values)
    return columns
