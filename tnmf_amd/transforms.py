"""
Transform groups of the factorisation (``TransformInvariantNMF(..., transforms=...)``): rotations by multiples of 90
degrees and mirrors of the atoms.  Each is an exact permutation of an atom's pixels, so a dictionary W of M atoms stands
for M * T effective atoms ``W_eff[m * T + t] = T_t(W[m])`` and the shift-invariant machinery runs unchanged on them; the W
half step folds the gradient of W_eff back onto W with the inverse permutations (the adjoint of the expansion).

A transform is coded as three bits (the codes of include/tnmf_hip.h's tables, tnmf_amd/csrc/group.hip):
``out[y, x] = a[sy, sx]`` with ``(u, v) = (x, y) if SWAP else (y, x)``, ``sy = Ay-1-u if FLIP_Y else u``,
``sx = Ax-1-v if FLIP_X else v``.  One shift axis: the atom is a single row (Ay = 1).

Atom operators (``AtomOperators``) widen the groups to any T non-negative linear maps L_t of an atom's
pixels -- rotations by arbitrary angles, rescalings, their products -- with ``W_eff[m * T + t, c] = L_t W[m, c]``: the same
model, with expand and fold small sparse gathers instead of permutations (fold is the transpose).  The weights are float64;
expand and fold sum the products of an output element in double, in the order of the operator's table, and round once.
"""
import hashlib
import math
from typing import Optional, Sequence, Tuple, Union

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


def check(transforms, atom_shape: Sequence[int]) -> Union[None, str, 'AtomOperators']:
    """The group name or the ``AtomOperators`` of ``transforms`` for atoms of ``atom_shape`` (None: no transforms).  An
    unknown value, a group of two shift axes on one, rotations of non-square atoms, or operators of another atom shape
    raise ValueError; three shift axes raise NotImplementedError."""
    if transforms is None:
        return None
    is_ops = isinstance(transforms, AtomOperators)
    if not is_ops and (not isinstance(transforms, str) or transforms not in GROUPS):
        raise ValueError(f'transforms must be None, an AtomOperators or one of {sorted(GROUPS)}, not {transforms!r}')
    k = len(atom_shape)
    if k == 3:
        raise NotImplementedError(f'transforms={transforms!r}: transforms cover 1 or 2 shift axes, not volumes')
    if is_ops:
        if transforms.atom_shape != tuple(atom_shape):
            raise ValueError(f'transforms: operators on atoms of shape {transforms.atom_shape}, the model\'s atoms are '
                             f'{tuple(atom_shape)}')
        return transforms
    if k == 1 and transforms in TWO_AXES_ONLY:
        raise ValueError(f'transforms={transforms!r} needs two shift axes; one shift axis has only "flip"')
    if transforms in SQUARE_ONLY and atom_shape[0] != atom_shape[1]:
        raise ValueError(f'transforms={transforms!r} needs square atoms, not {tuple(atom_shape)}')
    return transforms


def size(transforms) -> int:
    """T, the number of transforms of the group (the identity included) or of the operators."""
    if isinstance(transforms, AtomOperators):
        return transforms.T
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


def expand(W: np.ndarray, transforms) -> np.ndarray:
    """W[M, C, *A] -> W_eff[M * T, C, *A]."""
    if isinstance(transforms, AtomOperators):
        return transforms.expand(W)
    out = np.stack([apply(code, W) for code in GROUPS[transforms]], axis=1)
    return np.ascontiguousarray(out.reshape((-1,) + W.shape[1:]))


def fold(X: np.ndarray, transforms) -> np.ndarray:
    """X[M * T, C, *A] -> sum_t T_t^-1(X[m * T + t]) of shape [M, C, *A] (the adjoint of expand), summed in ascending t;
    for operators sum_t L_t^T X[m * T + t]."""
    if isinstance(transforms, AtomOperators):
        return transforms.fold(X)
    codes = GROUPS[transforms]
    Xt = X.reshape((-1, len(codes)) + X.shape[1:])
    out = apply_inverse(codes[0], Xt[:, 0]).copy()
    for t in range(1, len(codes)):
        out += apply_inverse(codes[t], Xt[:, t])
    return out



# -- atom operators ---------------------------------------------------------------------------------------------------------
SNAP = 1e-9        # a sample coordinate this close to an integer is that integer
DROP = 1e-12       # built-in weights below this are dropped


def _csr(keys: np.ndarray, n_rows: int) -> np.ndarray:
    """Row pointer of entries sorted by row ``keys``."""
    return np.concatenate([[0], np.cumsum(np.bincount(keys, minlength=n_rows))]).astype(np.int64)


def _padded(ptr: np.ndarray, *cols: np.ndarray):
    """Entries of a CSR table as [rows, width] arrays (width: the longest row) plus the mask of the real ones."""
    n_rows, lens = len(ptr) - 1, np.diff(ptr)
    width = int(lens.max()) if n_rows and lens.size else 0
    k = np.arange(width)
    mask = k[None, :] < lens[:, None]
    idx = np.where(mask, ptr[:-1, None] + k[None, :], 0)
    return mask, [c[idx] if c.size else np.zeros(idx.shape, c.dtype) for c in cols]


class AtomOperators:
    """T non-negative linear maps L_t of the pixels of an atom of ``atom_shape`` (the same map for every channel), held
    sparse as entries (t, out pixel, in pixel, weight): ``(L_t a)[out] = sum weight * a[in]``.  Pixels are flat C-order
    indices of the atom.  Immutable; the entries are kept sorted by (t, out, in), every triple once, weights float64,
    finite and > 0.  Build one with ``from_dense``, ``rotations``, ``scales``, ``compose`` or ``from_group``."""

    __slots__ = ('_atom_shape', '_T', '_t', '_out', '_in', '_w', '_key')

    def __init__(self, atom_shape: Sequence[int], T: int, t, out_px, in_px, w):
        atom_shape = tuple(int(a) for a in atom_shape)
        if not 1 <= len(atom_shape) <= 3 or min(atom_shape) <= 0:
            raise ValueError(f'atom_shape must have 1 to 3 positive sizes, not {atom_shape}')
        if int(T) != T or T < 1:
            raise ValueError(f'T must be a positive integer, not {T!r}')
        T, nA = int(T), int(np.prod(atom_shape))
        t, out_px, in_px = (np.asarray(x, dtype=np.int64).ravel() for x in (t, out_px, in_px))
        w = np.asarray(w, dtype=np.float64).ravel()
        if not len(t) == len(out_px) == len(in_px) == len(w):
            raise ValueError('t, out_px, in_px and w must have one entry each')
        if len(t) and (t.min() < 0 or t.max() >= T or min(out_px.min(), in_px.min()) < 0
                       or max(out_px.max(), in_px.max()) >= nA):
            raise ValueError(f'an entry indexes outside T = {T} maps of {nA} pixels')
        if not np.all(np.isfinite(w)) or np.any(w < 0):
            raise ValueError('the weights must be finite and non-negative')
        keep = w > 0
        t, out_px, in_px, w = t[keep], out_px[keep], in_px[keep], w[keep]
        order = np.lexsort((in_px, out_px, t))
        t, out_px, in_px, w = t[order], out_px[order], in_px[order], w[order]
        flat = (t * nA + out_px) * nA + in_px
        if np.any(flat[1:] == flat[:-1]):
            raise ValueError('an entry (t, out pixel, in pixel) occurs twice')
        for a in (t, out_px, in_px, w):
            a.flags.writeable = False
        self._atom_shape, self._T = atom_shape, T
        self._t, self._out, self._in, self._w = t, out_px, in_px, w
        h = hashlib.sha256(repr((atom_shape, T)).encode())
        for a in (t, out_px, in_px, w):
            h.update(a.tobytes())
        self._key = h.hexdigest()

    def __setattr__(self, name, value):
        if hasattr(self, '_key'):
            raise AttributeError('AtomOperators is immutable')
        object.__setattr__(self, name, value)

    # -- the value --------------------------------------------------------------------------------------------------
    @property
    def atom_shape(self) -> Tuple[int, ...]:
        return self._atom_shape

    @property
    def T(self) -> int:
        """The number of maps."""
        return self._T

    @property
    def n_pixels(self) -> int:
        return int(np.prod(self._atom_shape))

    @property
    def nnz(self) -> int:
        return len(self._w)

    @property
    def entries(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        """(t, out pixel, in pixel, weight), sorted by (t, out, in) (read-only arrays)."""
        return self._t, self._out, self._in, self._w

    @property
    def key(self) -> str:
        """A digest of the atom shape, T and the entries: equal operators have equal keys."""
        return self._key

    def __eq__(self, other):
        return isinstance(other, AtomOperators) and other._key == self._key

    def __hash__(self):
        return hash(self._key)

    def __repr__(self):
        return f'AtomOperators(atom_shape={self._atom_shape}, T={self._T}, nnz={self.nnz})'

    def dense(self) -> np.ndarray:
        """L as a float64 array [T, *A, *A] (output pixel axes first)."""
        nA = self.n_pixels
        L = np.zeros((self._T, nA, nA))
        L[self._t, self._out, self._in] = self._w
        return L.reshape((self._T,) + self._atom_shape * 2)

    # -- expand and its adjoint (float64; products summed in table order, as the library does) -----------------------
    def _forward(self):
        """Per (t, out pixel): the taps in ascending in pixel, padded -> (mask, in pixel, weight) of [T * nA, width]."""
        return _padded(_csr(self._t * self.n_pixels + self._out, self._T * self.n_pixels), self._in, self._w)

    def _adjoint(self):
        """Per in pixel: the entries in ascending (t, out pixel), padded -> (mask, t, out pixel, weight) of [nA, width]."""
        order = np.argsort(self._in, kind='stable')     # (stable: (t, out) stays ascending within an in pixel)
        return _padded(_csr(self._in[order], self.n_pixels), self._t[order], self._out[order], self._w[order])

    def expand(self, W: np.ndarray) -> np.ndarray:
        """W[M, C, *A] -> W_eff[M * T, C, *A], W_eff[m * T + t, c] = L_t W[m, c], in float64 rounded once to W's dtype."""
        M, C, nA, T = W.shape[0], W.shape[1], self.n_pixels, self._T
        assert tuple(W.shape[2:]) == self._atom_shape
        X = np.asarray(W, dtype=np.float64).reshape(M, C, nA)
        mask, (src, w) = self._forward()
        out = np.zeros((M, C, T * nA))
        for k in range(mask.shape[1]):
            out += np.where(mask[:, k], w[:, k] * X[:, :, src[:, k]], 0.)
        out = out.reshape(M, C, T, nA).transpose(0, 2, 1, 3)
        return np.ascontiguousarray(out.reshape((M * T, C) + self._atom_shape), dtype=W.dtype)

    def fold(self, X: np.ndarray) -> np.ndarray:
        """X[M * T, C, *A] -> [M, C, *A], sum_t L_t^T X[m * T + t] (the adjoint of expand), in float64 rounded once."""
        T, nA = self._T, self.n_pixels
        assert X.shape[0] % T == 0 and tuple(X.shape[2:]) == self._atom_shape
        M, C = X.shape[0] // T, X.shape[1]
        Y = np.asarray(X, dtype=np.float64).reshape(M, T, C, nA)
        mask, (t, q, w) = self._adjoint()
        out = np.zeros((M, C, nA))
        for k in range(mask.shape[1]):
            out += np.where(mask[:, k], w[:, k] * Y[:, t[:, k], :, q[:, k]].transpose(1, 2, 0), 0.)
        return out.reshape((M, C) + self._atom_shape).astype(X.dtype)

    # -- constructors ---------------------------------------------------------------------------------------------------
    @classmethod
    def from_dense(cls, L) -> 'AtomOperators':
        """From L of shape [T, *A, *A] (output pixel axes first), finite and >= 0."""
        L = np.asarray(L)
        if L.dtype.kind not in 'fiu' or L.ndim not in (3, 5, 7):
            raise ValueError(f'L must be a real array [T, *A, *A] with 1 to 3 atom axes, not of shape {L.shape}')
        k = (L.ndim - 1) // 2
        A = L.shape[1:1 + k]
        if L.shape[1 + k:] != A or L.shape[0] < 1 or min(A) < 1:
            raise ValueError(f'L must have the shape [T, *A, *A], not {L.shape}')
        L = L.astype(np.float64)
        if not np.all(np.isfinite(L)) or np.any(L < 0):
            raise ValueError('L must be finite and non-negative')
        nA = int(np.prod(A))
        t, o, i = np.nonzero(L.reshape(L.shape[0], nA, nA))
        return cls(A, L.shape[0], t, o, i, L.reshape(L.shape[0], nA, nA)[t, o, i])

    @classmethod
    def from_group(cls, name: str, atom_shape: Sequence[int]) -> 'AtomOperators':
        """A permutation group of tnmf_amd/transforms.py as operators, in the group's t order (weight 1, one tap)."""
        name = check(name, atom_shape)
        if not isinstance(name, str):
            raise ValueError(f'from_group takes a group name, not {name!r}')
        A = tuple(atom_shape)
        nA = int(np.prod(A))
        idx = np.arange(nA).reshape(A if len(A) == 2 else (1,) + A)
        t, o, i = [], [], []
        for k, code in enumerate(GROUPS[name]):
            src = np.ascontiguousarray(apply(code, idx)).ravel()
            t.append(np.full(nA, k))
            o.append(np.arange(nA))
            i.append(src)
        return cls(A, len(GROUPS[name]), np.concatenate(t), np.concatenate(o), np.concatenate(i), np.ones(len(GROUPS[name]) * nA))


def _resample(atom_shape: Sequence[int], maps) -> AtomOperators:
    """Operators of output pixel p sampling the atom at ``c + R(-theta) (p - c) / s`` (c: the atom centre), bilinear (1-D:
    linear) with the source outside the atom contributing 0; for s < 1 every output pixel averages the samples at an
    n x n grid of sub-points (n = ceil(1/s) per axis).  ``maps``: (theta, s) per t."""
    A = tuple(int(a) for a in atom_shape)
    one_d = len(A) == 1
    Ay, Ax = (1, A[0]) if one_d else A
    cy, cx = (Ay - 1) / 2., (Ax - 1) / 2.
    nA = Ay * Ax
    t_all, o_all, i_all, w_all = [], [], [], []
    for t, (theta, s) in enumerate(maps):
        n = max(1, int(math.ceil(1. / s - SNAP)))
        sub = (np.arange(n) + 0.5) / n - 0.5                     # sub-point offsets within a pixel (0 for n = 1)
        py, px = np.meshgrid(np.arange(Ay, dtype=np.float64), np.arange(Ax, dtype=np.float64), indexing='ij')
        oy, ox = np.meshgrid(sub, sub, indexing='ij')
        if one_d:
            oy = np.zeros_like(ox[:1])
            ox = sub[None, :]
        dy = (py.ravel()[:, None] + oy.ravel()[None, :]) - cy    # [nA, sub-points]
        dx = (px.ravel()[:, None] + ox.ravel()[None, :]) - cx
        ct, st = math.cos(theta), math.sin(theta)
        sy = cy + (ct * dy + st * dx) / s
        sx = cx + (-st * dy + ct * dx) / s
        for v in (sy, sx):
            r = np.round(v)
            snap = np.abs(v - r) <= SNAP
            v[snap] = r[snap]
        y0, x0 = np.floor(sy), np.floor(sx)
        fy, fx = sy - y0, sx - x0
        n_sub = sy.shape[1]
        out = np.repeat(np.arange(nA), n_sub)
        for ty, wy in ((0, 1. - fy), (1, fy)):
            for tx, wx in ((0, 1. - fx), (1, fx)):
                yy, xx = (y0 + ty).ravel(), (x0 + tx).ravel()
                w = (wy * wx).ravel() / n_sub
                ok = (yy >= 0) & (yy < Ay) & (xx >= 0) & (xx < Ax) & (w > 0)
                t_all.append(np.full(int(ok.sum()), t))
                o_all.append(out[ok])
                i_all.append((yy[ok] * Ax + xx[ok]).astype(np.int64))
                w_all.append(w[ok])
    t, o, i, w = (np.concatenate(x) for x in (t_all, o_all, i_all, w_all))
    # sum the taps of one (t, out, in) (several sub-points and corners meet on a source pixel), in a fixed order
    key = (t * nA + o) * nA + i
    uniq, inv = np.unique(key, return_inverse=True)
    ws = np.bincount(inv, weights=w, minlength=len(uniq))
    keep = ws >= DROP
    uniq, ws = uniq[keep], ws[keep]
    return AtomOperators(A, len(maps), uniq // (nA * nA), (uniq // nA) % nA, uniq % nA, ws)


def rotations(atom_shape: Sequence[int], n: int) -> AtomOperators:
    """T = n rotations by the angles 2 pi t / n, t = 0..n-1 (bilinear; 2 shift axes; 90 degrees is ``np.rot90(a, 1)``)."""
    if len(atom_shape) != 2:
        raise ValueError(f'rotations need 2 shift axes, not atoms of shape {tuple(atom_shape)}')
    if int(n) != n or n < 1:
        raise ValueError(f'n must be a positive integer, not {n!r}')
    return _resample(atom_shape, [(2. * math.pi * t / int(n), 1.) for t in range(int(n))])


def scales(atom_shape: Sequence[int], factors: Sequence[float]) -> AtomOperators:
    """T = len(factors) rescalings about the atom centre by s (s > 1 magnifies; s < 1 shrinks, averaging ceil(1/s)
    sub-points per axis); 1 or 2 shift axes."""
    if len(atom_shape) not in (1, 2):
        raise ValueError(f'scales need 1 or 2 shift axes, not atoms of shape {tuple(atom_shape)}')
    factors = [float(s) for s in np.atleast_1d(np.asarray(factors, dtype=np.float64))]
    if not factors or not all(math.isfinite(s) and s > 0 for s in factors):
        raise ValueError(f'scale factors must be finite and > 0, not {factors!r}')
    return _resample(atom_shape, [(0., s) for s in factors])


def compose(outer: AtomOperators, inner: AtomOperators) -> AtomOperators:
    """T = T_outer * T_inner maps ``[i * T_inner + j] = outer[i] o inner[j]`` (inner applied first)."""
    if not isinstance(outer, AtomOperators) or not isinstance(inner, AtomOperators):
        raise ValueError('compose takes two AtomOperators')
    if outer.atom_shape != inner.atom_shape:
        raise ValueError(f'compose: atom shapes {outer.atom_shape} and {inner.atom_shape} differ')
    nA, Ti = outer.n_pixels, inner.T
    ot, oo, oi, ow = outer.entries
    it, io, ii, iw = inner.entries
    t_all, key_all, w_all = [], [], []
    for j in range(Ti):
        sel = it == j                                           # inner[j]: rows io -> columns ii (sorted by io)
        jo, ji, jw = io[sel], ii[sel], iw[sel]
        ptr = _csr(jo, nA)
        cnt = np.diff(ptr)[oi]                                  # every outer entry (o, k) meets inner row k
        rep = np.repeat(np.arange(len(ow)), cnt)
        pos = np.repeat(ptr[oi], cnt) + (np.arange(len(rep)) - np.repeat(np.cumsum(cnt) - cnt, cnt))
        t = ot[rep] * Ti + j
        t_all.append(t)
        key_all.append((t * nA + oo[rep]) * nA + ji[pos])
        w_all.append(ow[rep] * jw[pos])
    key, w = np.concatenate(key_all), np.concatenate(w_all)
    uniq, inv = np.unique(key, return_inverse=True)
    ws = np.bincount(inv, weights=w, minlength=len(uniq))
    keep = ws >= DROP
    uniq, ws = uniq[keep], ws[keep]
    return AtomOperators(outer.atom_shape, outer.T * Ti, uniq // (nA * nA), (uniq // nA) % nA, uniq % nA, ws)


def from_group(name: str, atom_shape: Sequence[int]) -> AtomOperators:
    """The permutation group ``name`` on atoms of ``atom_shape`` as operators, in the same t order."""
    return AtomOperators.from_group(name, atom_shape)
