"""
The checks of scalar arguments the front end shares: each raises ``ValueError('{name} must be ..., not {value!r}')``.

A bool (``bool``, ``np.bool_``) is not a number here; NumPy's integer and floating scalars are, through ``numbers.Integral``
and ``numbers.Real``; NaN and +-inf are not finite numbers.
"""
import math
import numbers

import numpy as np


def is_bool(value) -> bool:
    return isinstance(value, (bool, np.bool_))


def is_int(value) -> bool:
    return isinstance(value, numbers.Integral) and not is_bool(value)


def is_real(value) -> bool:
    return isinstance(value, numbers.Real) and not is_bool(value)


def _refuse(name: str, kind: str, value, none_ok: bool):
    raise ValueError(f'{name} must be {"None or " if none_ok else ""}{kind}, not {value!r}')


def int_at_least(name: str, value, lo: int, none_ok: bool = False) -> None:
    """``value`` is an int >= ``lo`` (or, with ``none_ok``, None)."""
    if not (none_ok and value is None) and (not is_int(value) or value < lo):
        _refuse(name, f'an int >= {lo}', value, none_ok)


def finite_number(name: str, value, bound: str = None, none_ok: bool = False) -> None:
    """``value`` is a finite real number within ``bound`` -- None, ``'>= 0'`` or ``'> 0'`` -- (or, with ``none_ok``, None)."""
    if none_ok and value is None:
        return
    within = {None: lambda x: True, '>= 0': lambda x: x >= 0, '> 0': lambda x: x > 0}[bound]
    if not is_real(value) or not math.isfinite(value) or not within(value):
        _refuse(name, 'a finite number' + ('' if bound is None else ' ' + bound), value, none_ok)


def one_of(name: str, value, choices) -> None:
    """``value`` is one of the strings ``choices``."""
    if not isinstance(value, str) or value not in choices:
        _refuse(name, 'one of ' + ', '.join(repr(c) for c in choices), value, False)


def disjoint_index_sets(name: str, value, n: int) -> list:
    """``value`` is a non-empty sequence of non-empty sequences of ints in ``[0, n)``, no int in two of them or twice in
    one -> the sets as lists of Python ints."""
    kind = f'a sequence of disjoint, non-empty sequences of ints in [0, {n})'
    try:
        sets = [list(one) for one in value]
    except TypeError:
        _refuse(name, kind, value, False)
    seen = set()
    for one in sets:
        if not one:
            _refuse(name, kind, value, False)
        for m in one:
            if not is_int(m) or not 0 <= m < n or int(m) in seen:
                _refuse(name, kind, value, False)
            seen.add(int(m))
    if not sets:
        _refuse(name, kind, value, False)
    return [[int(m) for m in one] for one in sets]


def boolean(name: str, value) -> None:
    if not is_bool(value):
        _refuse(name, 'a bool', value, False)
