"""
Transform groups of the factorisation (``TransformInvariantNMF(..., transforms=...)``): rotations by multiples of 90
degrees and mirrors of the atoms.  Each is an exact permutation of an atom's pixels, so a dictionary W of M atoms stands
for M * T effective atoms ``W_eff[m * T + t] = T_t(W[m])`` and the shift-invariant machinery runs unchanged on them; the W
half step folds the gradient of W_eff back onto W with the inverse permutations (the adjoint of the expansion).

A transform is coded as three bits (the codes of include/tnmf_hip.h's tables, tnmf_amd/csrc/group.hip):
``out[y, x] = a[sy, sx]`` with ``(u, v) = (x, y) if SWAP else (y, x)``, ``sy = Ay-1-u if FLIP_Y else u``,
``sx = Ax-1-v if FLIP_X else v``.  One shift axis: the atom is a single row (Ay = 1).
"""
from typing import Optional, Sequence

import numpy as np

FLIP_X, FLIP_Y, SWAP = 1, 2, 4

# name -> codes of T_t, t = 0..T-1 (the order of the public interface)
GROUPS = {
    'flip': (0, FLIP_X),                                                    # a, a[..., ::-1]
    'mirrors': (0, FLIP_X, FLIP_Y, FLIP_Y | FLIP_X),                        # a, a[:, ::-1], a[::-1, :], a[::-1, ::-1]
    'rot90': (0, SWAP | FLIP_X, FLIP_Y | FLIP_X, SWAP | FLIP_Y),            # np.rot90(a, k), k = 0..3
    'dihedral': (0, SWAP | FLIP_X, FLIP_Y | FLIP_X, SWAP | FLIP_Y,          # np.rot90(a, k), then
                 FLIP_X, SWAP, FLIP_Y, SWAP | FLIP_Y | FLIP_X),             # np.rot90(a[:, ::-1], k), k = 0..3
}
TWO_AXES_ONLY = ('mirrors', 'rot90', 'dihedral')
SQUARE_ONLY = ('rot90', 'dihedral')


def check(transforms, atom_shape: Sequence[int]) -> Optional[str]:
    """The group name of ``transforms`` for atoms of ``atom_shape`` (None: no transforms).  An unknown value, a group of two
    shift axes on one, or rotations of non-square atoms raise ValueError; three shift axes raise NotImplementedError."""
    if transforms is None:
        return None
    if not isinstance(transforms, str) or transforms not in GROUPS:
        raise ValueError(f'transforms must be None or one of {sorted(GROUPS)}, not {transforms!r}')
    k = len(atom_shape)
    if k == 3:
        raise NotImplementedError(f'transforms={transforms!r}: transforms cover 1 or 2 shift axes, not volumes')
    if k == 1 and transforms in TWO_AXES_ONLY:
        raise ValueError(f'transforms={transforms!r} needs two shift axes; one shift axis has only "flip"')
    if transforms in SQUARE_ONLY and atom_shape[0] != atom_shape[1]:
        raise ValueError(f'transforms={transforms!r} needs square atoms, not {tuple(atom_shape)}')
    return transforms


def size(transforms: str) -> int:
    """T, the number of transforms of the group (the identity included)."""
    return len(GROUPS[transforms])


def apply(code: int, a: np.ndarray) -> np.ndarray:
    """T_code over the last two axes of ``a`` (one axis: the last, as a single row): the flips of the source, then the
    transpose."""
    if code & FLIP_Y:
        a = a[..., ::-1, :]
    if code & FLIP_X:
        a = a[..., ::-1]
    if code & SWAP:
        a = np.swapaxes(a, -1, -2)
    return a


def apply_inverse(code: int, a: np.ndarray) -> np.ndarray:
    """T_code^-1 over the last two axes of ``a``."""
    if code & SWAP:
        a = np.swapaxes(a, -1, -2)
    if code & FLIP_X:
        a = a[..., ::-1]
    if code & FLIP_Y:
        a = a[..., ::-1, :]
    return a


def expand(W: np.ndarray, transforms: str) -> np.ndarray:
    """W[M, C, *A] -> W_eff[M * T, C, *A]."""
    out = np.stack([apply(code, W) for code in GROUPS[transforms]], axis=1)
    return np.ascontiguousarray(out.reshape((-1,) + W.shape[1:]))


def fold(X: np.ndarray, transforms: str) -> np.ndarray:
    """X[M * T, C, *A] -> sum_t T_t^-1(X[m * T + t]) of shape [M, C, *A] (the adjoint of expand), summed in ascending t."""
    codes = GROUPS[transforms]
    Xt = X.reshape((-1, len(codes)) + X.shape[1:])
    out = apply_inverse(codes[0], Xt[:, 0]).copy()
    for t in range(1, len(codes)):
        out += apply_inverse(codes[t], Xt[:, t])
    return out

