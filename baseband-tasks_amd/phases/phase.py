"""Two-part pulse phase: whole cycles and a fraction in [-0.5, 0.5], both float64
(the reference's `baseband_tasks.phases.Phase`, without the astropy `Angle` and
ufunc surface: plain NumPy, the unit is always cycles).

Sums, differences and products with plain numbers are carried out with
error-free transformations (Knuth's two-sum, Dekker's split product), so a phase
of 1e11 cycles keeps its fraction to ~1e-16 cycle.
"""
import numbers

import numpy as np

__all__ = ['Phase']


def _two_sum(a, b):
    """a + b as (rounded sum, exact error)."""
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _split(a):
    c = 134217729. * a                      # 2**27 + 1
    hi = c - (c - a)
    return hi, a - hi


def _two_product(a, b):
    """a * b as (rounded product, exact error)."""
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def _count_frac(v1, v2=0., factor=None, divisor=None):
    """(v1 + v2) [* factor] [/ divisor] as (nearest whole number, remainder in [-0.5, 0.5])."""
    v1 = np.asarray(v1, dtype=float)
    v2 = np.asarray(v2, dtype=float)
    total, err = _two_sum(v1, v2)
    if factor is not None:
        factor = np.asarray(factor, dtype=float)
        total, carry = _two_product(total, factor)
        carry = carry + err * factor
        total, err = _two_sum(total, carry)
    if divisor is not None:
        divisor = np.asarray(divisor, dtype=float)
        q1 = total / divisor
        p1, p2 = _two_product(q1, divisor)
        d1, d2 = _two_sum(total, -p1)
        d2 = (d2 + err) - p2
        q2 = (d1 + d2) / divisor
        total, err = _two_sum(q1, q2)
    count = np.round(total)
    extra, frac = _two_sum(total, -count)
    frac = frac + (extra + err)
    # the remainder may have rounded out of range: once more
    excess = np.round(frac)
    count = count + excess
    extra, frac = _two_sum(total, -count)
    frac = frac + (extra + err)
    return count, frac


def _parse_decimal(text):
    """Decimal string -> (digits before the point, digits after it) as two doubles, the
    exponent (``e`` or Fortran's ``d``) applied by moving the point."""
    s = text.strip().lower().replace('d', 'e')
    sign = 1.
    if s[:1] in '+-':
        sign = -1. if s[0] == '-' else 1.
        s = s[1:]
    float(s)                                    # (raises ValueError for anything not a number)
    mantissa, _, exponent = s.partition('e')
    whole, _, rest = mantissa.partition('.')
    shift = int(exponent) if exponent else 0
    if shift > 0:
        rest = rest.ljust(shift, '0')
        whole, rest = whole + rest[:shift], rest[shift:]
    elif shift < 0:
        whole = whole.rjust(-shift, '0')
        whole, rest = whole[:shift], whole[shift:] + rest
    return sign * float('0' + whole), sign * float('0.' + rest + '0')


def _values(x):
    """Cycles of a number, array, string(s) or anything with ``to_value('cycle')``, as the
    pair of doubles that `_count_frac` adds."""
    if hasattr(x, 'to_value') and not isinstance(x, Phase):
        x = x.to_value('cycle')
    a = np.asarray(x)
    if a.dtype.kind in 'SU':
        parts = np.array([_parse_decimal(str(s)) for s in a.astype(str).ravel()], dtype=float)
        return parts[:, 0].reshape(a.shape), parts[:, 1].reshape(a.shape)
    return a.astype(float), np.zeros((), float)


class Phase:
    """Phase in cycles as two float64 parts.

    Parameters
    ----------
    phase1, phase2 : number, array, decimal string(s) or `Phase`
        Their sum is the phase.  A string keeps the digits after its decimal point at full
        precision (``Phase('162169181660.066162')``; `from_string` is the same).

    Attributes
    ----------
    int : whole cycles (float64, the nearest whole number)
    frac : the rest, in [-0.5, 0.5]

    ``+`` and ``-`` (with phases or numbers), negation, ``*`` and ``/`` by plain numbers
    keep the precision; comparisons compare the exact difference with zero.
    ``to_value('cycle')`` / ``.cycle`` / ``.value`` give one float64 (and lose it).
    """
    __slots__ = ('int', 'frac')
    __array_priority__ = 20000                  # (ndarray <op> Phase -> Phase.__r<op>__)
    __array_ufunc__ = None

    def __init__(self, phase1, phase2=None):
        if isinstance(phase1, Phase) and phase2 is None:
            self.int, self.frac = phase1.int.copy(), phase1.frac.copy()
            return
        parts = []
        for p in (phase1, phase2):
            if p is None:
                continue
            if isinstance(p, Phase):
                parts.append((p.int, p.frac))
            else:
                parts.append(_values(p))
        count, frac = _count_frac(parts[0][0], parts[0][1])
        for a, b in parts[1:]:
            c2, f2 = _count_frac(a, b)
            count, frac = self._combine(count, frac, c2, f2)
        self.int, self.frac = count, frac

    @staticmethod
    def _combine(c1, f1, c2, f2):
        """(c1 + f1) + (c2 + f2): whole numbers add exactly (below 2**53)."""
        extra, frac = _count_frac(f1, f2)
        return (c1 + c2) + extra, frac

    @classmethod
    def _from_parts(cls, count, frac):
        self = object.__new__(cls)
        self.int, self.frac = np.asarray(count, dtype=float), np.asarray(frac, dtype=float)
        return self

    @classmethod
    def from_string(cls, string):
        """Phase from (an array of) decimal strings, at the full precision of the digits."""
        a = np.asarray(string)
        if a.dtype.kind not in 'SU':
            raise ValueError('require string input.')
        return cls(a)

    # -- values -----------------------------------------------------------------------
    @property
    def cycle(self):
        return self.int + self.frac

    value = cycle

    def to_value(self, unit='cycle'):
        if str(unit) not in ('cycle', 'cy', '1.0'):
            raise ValueError("a Phase is in cycles")
        return self.cycle

    @property
    def shape(self):
        return np.shape(self.int)

    @property
    def ndim(self):
        return np.ndim(self.int)

    @property
    def size(self):
        return np.size(self.int)

    @property
    def isscalar(self):
        return self.ndim == 0

    def __len__(self):
        if self.isscalar:
            raise TypeError("scalar Phase has no len()")
        return len(self.int)

    def __getitem__(self, item):
        if isinstance(item, str):
            if item not in ('int', 'frac'):
                raise KeyError(item)
            return getattr(self, item)
        if self.isscalar:
            raise TypeError("scalar Phase cannot be indexed")
        return Phase._from_parts(self.int[item], self.frac[item])

    def __iter__(self):
        if self.isscalar:
            raise TypeError("scalar Phase is not iterable")
        return (self[i] for i in range(len(self)))

    def reshape(self, *shape):
        return Phase._from_parts(self.int.reshape(*shape), self.frac.reshape(*shape))

    def ravel(self):
        return Phase._from_parts(self.int.ravel(), self.frac.ravel())

    def copy(self):
        return Phase._from_parts(self.int.copy(), self.frac.copy())

    # -- arithmetic -------------------------------------------------------------------
    @staticmethod
    def _coerce(other):
        if isinstance(other, Phase):
            return other
        if isinstance(other, (numbers.Real, np.ndarray, list, tuple, str)) or hasattr(other, 'to_value'):
            try:
                return Phase(other)
            except (TypeError, ValueError):
                return None
        return None

    def __add__(self, other):
        other = self._coerce(other)
        if other is None:
            return NotImplemented
        return Phase._from_parts(*self._combine(self.int, self.frac, other.int, other.frac))

    __radd__ = __add__

    def __neg__(self):
        return Phase._from_parts(-self.int, -self.frac)

    def __pos__(self):
        return self.copy()

    def __sub__(self, other):
        other = self._coerce(other)
        if other is None:
            return NotImplemented
        return self + (-other)

    def __rsub__(self, other):
        other = self._coerce(other)
        if other is None:
            return NotImplemented
        return other + (-self)

    @staticmethod
    def _number(x):
        if isinstance(x, Phase) or isinstance(x, str):
            return None
        try:
            a = np.asarray(x, dtype=float)
        except (TypeError, ValueError):
            return None
        return a

    def __mul__(self, factor):
        factor = self._number(factor)
        if factor is None:
            return NotImplemented
        return Phase._from_parts(*_count_frac(self.int, self.frac, factor=factor))

    __rmul__ = __mul__

    def __truediv__(self, divisor):
        divisor = self._number(divisor)
        if divisor is None:
            return NotImplemented
        return Phase._from_parts(*_count_frac(self.int, self.frac, divisor=divisor))

    def __abs__(self):
        neg = self.cycle < 0
        return Phase._from_parts(np.where(neg, -self.int, self.int), np.where(neg, -self.frac, self.frac))

    # -- comparisons (of the exact difference with zero) ----------------------------------
    def _diff(self, other):
        other = self._coerce(other)
        if other is None:
            return None
        return (self.int - other.int) + (self.frac - other.frac)

    def __eq__(self, other):
        d = self._diff(other)
        return NotImplemented if d is None else d == 0

    def __ne__(self, other):
        d = self._diff(other)
        return NotImplemented if d is None else d != 0

    def __lt__(self, other):
        d = self._diff(other)
        return NotImplemented if d is None else d < 0

    def __le__(self, other):
        d = self._diff(other)
        return NotImplemented if d is None else d <= 0

    def __gt__(self, other):
        d = self._diff(other)
        return NotImplemented if d is None else d > 0

    def __ge__(self, other):
        d = self._diff(other)
        return NotImplemented if d is None else d >= 0

    __hash__ = None

    def min(self):
        return self.ravel()[int(np.lexsort((self.frac.ravel(), self.int.ravel()))[0])]

    def max(self):
        return self.ravel()[int(np.lexsort((self.frac.ravel(), self.int.ravel()))[-1])]

    # -- text -------------------------------------------------------------------------
    def to_string(self, precision=None):
        """Decimal string(s) that keep both parts (``precision`` digits after the point;
        default: as many as the fraction needs)."""
        def one(count, frac):
            sign = ''
            if count + frac < 0:
                count, frac, sign = -count, -frac, '-'
            if frac < 0:
                count, frac = count - 1, frac + 1
            digits = repr(float(frac)) if precision is None else '%.*f' % (precision, frac)
            if 'e' in digits:                   # (tiny fraction: fixed notation)
                digits = '%.25f' % frac
                digits = digits.rstrip('0') or '0.0'
            if digits.startswith('1'):          # rounding spilled over
                count, digits = count + 1, '0' + digits[1:]
            return sign + str(int(count)) + digits[1:]
        out = np.vectorize(one, otypes=['U'])(self.int, self.frac)
        return out[()] if out.ndim == 0 else out

    def __format__(self, spec):
        if spec.endswith('f') and self.isscalar:
            head, _, tail = spec[:-1].partition('.')
            text = self.to_string(precision=int(tail) if tail else 6)
            return format(text, '>' + head) if head else text
        return format(self.cycle, spec)

    def __repr__(self):
        return f"Phase({self.int} cycle, {self.frac} cycle)"

    __str__ = __repr__
