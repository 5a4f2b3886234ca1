"""The argument checks of tnmf_amd/_args.py: per validator the values it takes, the values it refuses and the exact message.
The feature tests pin these messages by substrings only; this table is where a drift shows."""
import fractions

import numpy as np
import pytest

from tnmf_amd import _args

NAN, INF = float('nan'), float('inf')
BOOLS = [True, False, np.True_, np.False_]
NOT_NUMBERS = BOOLS + [None, '3', 1j, [1], (2,), np.array([1.])]

# (the check with its arguments after the value, what the message says it must be, accepted, rejected)
TABLE = {
    'int >= 0': (
        lambda v: _args.int_at_least('n_iterations', v, 0), 'n_iterations must be an int >= 0',
        [0, 1, 10 ** 20, np.int64(3), np.uint8(0), np.int32(7)],
        NOT_NUMBERS + [-1, np.int64(-1), 0., 3.0, np.float32(0.5), NAN, INF, fractions.Fraction(1, 2)]),
    'int >= 1': (
        lambda v: _args.int_at_least('max_component', v, 1), 'max_component must be an int >= 1',
        [1, 2048, np.int64(3)],
        NOT_NUMBERS + [0, -1, np.int64(0), 1., np.float32(0.5), NAN, INF]),
    'None or int >= 0': (
        lambda v: _args.int_at_least('max_per_sample', v, 0, none_ok=True), 'max_per_sample must be None or an int >= 0',
        [None, 0, 5, np.int64(3)],
        BOOLS + ['3', -1, 2.5, np.float32(0.5), NAN, INF]),
    'finite': (
        lambda v: _args.finite_number('min_gain', v), 'min_gain must be a finite number',
        [0, -1, -2.5, 1e300, np.int64(3), np.float32(0.5), np.float64(-0.), fractions.Fraction(1, 3)],
        NOT_NUMBERS + [NAN, INF, -INF, np.float32(NAN), np.float64(INF)]),
    'finite >= 0': (
        lambda v: _args.finite_number('sparsity_H', v, '>= 0'), 'sparsity_H must be a finite number >= 0',
        [0, 0., -0., 1, 2.5, np.int64(3), np.float32(0.5)],
        NOT_NUMBERS + [-1, -1e-300, np.float32(-0.5), NAN, INF, -INF]),
    'finite > 0': (
        lambda v: _args.finite_number('tol', v, '> 0'), 'tol must be a finite number > 0',
        [1, 1e-300, 2.5, np.int64(3), np.float32(0.5)],
        NOT_NUMBERS + [0, 0., -0., -1, NAN, INF, -INF]),
    'None or finite > 0': (
        lambda v: _args.finite_number('noise', v, '> 0', none_ok=True), 'noise must be None or a finite number > 0',
        [None, 1, 0.25, np.int64(3), np.float32(0.5)],
        BOOLS + ['3', 0, -1, NAN, INF]),
    'bool': (
        lambda v: _args.boolean('per_sample', v), 'per_sample must be a bool',
        BOOLS,
        [None, 0, 1, 1., 'True', np.int64(3), np.float32(0.5), NAN, INF, -1, [True]]),
}


@pytest.mark.parametrize('kind', list(TABLE))
def test_accepted_values_pass_and_return_nothing(kind):
    check, _, accepted, _ = TABLE[kind]
    for value in accepted:
        assert check(value) is None, value


@pytest.mark.parametrize('kind', list(TABLE))
def test_rejected_values_raise_the_exact_message(kind):
    check, must, _, rejected = TABLE[kind]
    for value in rejected:
        with pytest.raises(ValueError) as err:
            check(value)
        assert str(err.value) == f'{must}, not {value!r}', value


def test_the_table_holds_the_values_a_drift_would_show_on():
    """Every validator of a number sees a bool of each kind, a NumPy integer and floating scalar, NaN, inf, -1 and None --
    accepted or rejected, but never left out."""
    for kind, (_, _, accepted, rejected) in TABLE.items():
        seen = [repr(v) for v in accepted + rejected]
        for value in (True, np.True_, np.int64(3), np.float32(0.5), NAN, INF, -1, None):
            assert repr(value) in seen, (kind, value)


def test_none_is_a_value_only_with_none_ok():
    for check in (lambda v, **kw: _args.int_at_least('k', v, 0, **kw), lambda v, **kw: _args.finite_number('x', v, **kw)):
        assert check(None, none_ok=True) is None
        with pytest.raises(ValueError, match='must be a'):
            check(None)
        with pytest.raises(ValueError, match='must be None or a'):
            check('no', none_ok=True)


def test_the_predicates_of_the_checks_with_a_shape_of_their_own():
    """``is_bool`` / ``is_int`` / ``is_real`` (min_distance, atoms, beta_loss and the fit's tol build on them): a bool is
    neither an int nor a real number."""
    for value in BOOLS:
        assert _args.is_bool(value) and not _args.is_int(value) and not _args.is_real(value)
    for value in (0, -3, np.int64(3), np.uint8(1)):
        assert _args.is_int(value) and _args.is_real(value) and not _args.is_bool(value)
    for value in (0.5, np.float32(0.5), NAN, INF, fractions.Fraction(1, 2)):
        assert _args.is_real(value) and not _args.is_int(value)
    for value in (None, '1', 1j, [1]):
        assert not _args.is_int(value) and not _args.is_real(value) and not _args.is_bool(value)
